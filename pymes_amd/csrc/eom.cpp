// EOM-CCSD sigma build and diagonals on the engine (see eom.h).  Term by term this is pymes/solver/eom_ccsd.py:268-385 with
// every V.T product that does not depend on the trial vector hoisted into per-solve intermediates; the comments name the
// reference lines.  Pair layouts (ov x ov matrices): Xd[(a,i),(b,j)] = X[a,b,i,j], Xx[(a,j),(b,i)] = X[a,b,i,j].
#include "eom.h"

#include "../../include/pymes_amd.h"

#include <algorithm>
#include <cmath>
#include <initializer_list>
#include <optional>
#include <string>

namespace pymes {

// ---- temporaries and hoisted arrays come from the engine's scratch pool: a second solve on the same context (the warm
// start of a Davidson run, the next FEAST solve) finds the buffers of the first instead of paying hipMalloc again ----------
double* EomSigma::get(int64_t doubles) { return e.scratch_get(doubles); }
void EomSigma::put(double* p) { e.scratch_put(p); }
void EomSigma::trim() { e.scratch_trim(); }
double* EomSigma::keep(int64_t doubles) {
    double* p = e.scratch_get(doubles);
    owned_.push_back(p);
    return p;
}
struct EomSigma::Tmp {
    EomSigma& s;
    double* p;
    Tmp(EomSigma& s_, int64_t n) : s(s_), p(s_.get(n)) {}
    ~Tmp() { s.put(p); }
    Tmp(const Tmp&) = delete;
    Tmp& operator=(const Tmp&) = delete;
    operator double*() const { return p; }
};

namespace {
struct Ops {       // the three engine calls every term is made of, with the output allocated by the caller
    Engine& e;
    void C(double al, const TView& A, const char* sa, const TView& B, const char* sb, double be, const TView& Cv, const char* sc,
           const char* batch = "") const {
        e.contract(al, A, sa, B, sb, be, Cv, sc, batch);
    }
    void P(double al, const TView& in, const char* si, double be, const TView& out, const char* so) const {
        e.permute(al, in, si, be, out, so);
    }
    void L(double* out, std::initializer_list<const double*> xs, std::initializer_list<double> cs, int64_t n) const {
        const double* x[8];
        double c[8];
        int m = 0;
        auto ci = cs.begin();
        for (auto xp : xs) { x[m] = xp; c[m] = *ci++; ++m; }
        dev::lincomb(out, m, x, c, n, e.stream);
    }
};
inline TView mv(const double* p, std::initializer_list<int64_t> d) { return make_view(p, d); }
}  // namespace

TView EomSigma::V(const char* name) const { return e.block(pattern_of_name(name), dressed); }

bool EomSigma::exchange_symmetric(const double* x, int64_t d0, int64_t d2) const {
    const int64_t d[4] = {d0, d0, d2, d2};
    double out[2] = {0.0, 0.0};
    dev::exchange_asymmetry(x, x, d, out, e.stream);
    return std::isfinite(out[1]) && out[0] <= 1e-13 * std::max(1.0, out[1]);      // inf / NaN entries: never "symmetric"
}

int EomSigma::flags() const {
    return (v_sym ? 1 : 0) | (t_sym ? 2 : 0) | (hole_sym ? 4 : 0) | (fused_ok ? 8 : 0) | (many_ok ? 16 : 0);
}

EomSigma::~EomSigma() {
    for (double* p : owned_) e.scratch_put(p);        // (stream-ordered: whoever gets them next enqueues behind our last kernel)
}

// ---- hoisting: everything of eom_ccsd.py:288-373 that does not depend on (u1, u2) -----------------------------------------
EomSigma::EomSigma(Engine& eng, const double* f_host, const double* t2, bool dressed_)
    : e(eng), no(eng.no), nv(eng.nv), dressed(dressed_), T(t2) {
    if (!f_host || !t2) throw Error("eom sigma: null Fock matrix / amplitudes");
    const int64_t o = no, v = nv, n = o + v, ov = o * v, ov2 = ov * ov;
    const Ops q{e};
    try {
        std::vector<double> h(static_cast<size_t>(std::max(v * v, std::max(o * v, o * o))));     // (f_oo is the largest when no > nv)
        auto upload = [&](int64_t r0, int64_t nr, int64_t c0, int64_t nc, double sign, bool transposed = false) {
            for (int64_t r = 0; r < nr; ++r)
                for (int64_t c = 0; c < nc; ++c)
                    h[transposed ? c * nr + r : r * nc + c] = sign * f_host[(r0 + r) * n + c0 + c];
            double* d = keep(nr * nc);
            dev::memcpy_h2d(d, h.data(), sizeof(double) * nr * nc, e.stream);
            dev::stream_sync(e.stream);            // (h is reused)
            return d;
        };
        foo = upload(0, o, 0, o, 1.0);
        fov = upload(0, o, o, v, 1.0);
        fvv = upload(o, v, o, v, 1.0);
        const TView Vijab = V("ijab"), Viabj = V("iabj"), Viajb = V("iajb"), Vijka = V("ijka"), Vijak = V("ijak"),
                    Viabc = V("iabc"), Viajk = V("iajk"), Vklij = V("klij"), Vabcd = V("abcd");
        const TView T4 = mv(T, {v, v, o, o});
        Td = keep(ov2);
        Tx = keep(ov2);
        q.P(1.0, T4, "abij", 0.0, mv(Td, {v, o, v, o}), "aibj");
        q.P(1.0, T4, "abij", 0.0, mv(Tx, {v, o, v, o}), "ajbi");
        {
            Tmp Vd(*this, ov2), Vx(*this, ov2);
            q.P(1.0, Vijab, "klcd", 0.0, mv(Vd, {v, o, v, o}), "ckdl");          // [(c,k),(d,l)]
            q.P(1.0, Vijab, "klcd", 0.0, mv(Vx, {v, o, v, o}), "cldk");          // [(c,l),(d,k)]
            // ---- singles (eom_ccsd.py:288-308) ---------------------------------------------------------------------------
            // W1[(c,k),(a,i)] = sum_jb (2V[j,k,b,c]-V[j,k,c,b]) (2T[b,a,j,i]-T[a,b,j,i]) + 2V_iabj[k,a,c,i] - V_iajb[k,a,i,c]
            W1 = keep(ov2);
            {
                Tmp Vq(*this, ov2), Tq(*this, ov2);
                q.P(2.0, Vijab, "jkbc", 0.0, mv(Vq, {v, o, v, o}), "ckbj");
                q.P(-1.0, Vijab, "jkcb", 1.0, mv(Vq, {v, o, v, o}), "ckbj");
                q.P(2.0, T4, "baji", 0.0, mv(Tq, {v, o, v, o}), "bjai");
                q.P(-1.0, T4, "abji", 1.0, mv(Tq, {v, o, v, o}), "bjai");
                q.C(1.0, mv(Vq, {v, o, v, o}), "ckbj", mv(Tq, {v, o, v, o}), "bjai", 0.0, mv(W1, {v, o, v, o}), "ckai");
            }
            q.P(2.0, Viabj, "kaci", 1.0, mv(W1, {v, o, v, o}), "ckai");
            q.P(-1.0, Viajb, "kaic", 1.0, mv(W1, {v, o, v, o}), "ckai");
            // Gvv_s[a,c] = fvv + sum V[j,k,b,c] (-2T[b,a,j,k] + T[a,b,j,k]);  Goo_s[k,i] = -foo + sum (-2V[j,k,b,c]+V[j,k,c,b]) T[b,c,j,i]
            Gvv_s = keep(v * v);
            q.L(Gvv_s, {fvv}, {1.0}, v * v);
            q.C(-2.0, Vijab, "jkbc", T4, "bajk", 1.0, mv(Gvv_s, {v, v}), "ac");
            q.C(1.0, Vijab, "jkbc", T4, "abjk", 1.0, mv(Gvv_s, {v, v}), "ac");
            Goo_s = keep(o * o);
            q.L(Goo_s, {foo}, {-1.0}, o * o);
            q.C(-2.0, Vijab, "jkbc", T4, "bcji", 1.0, mv(Goo_s, {o, o}), "ki");
            q.C(1.0, Vijab, "jkcb", T4, "bcji", 1.0, mv(Goo_s, {o, o}), "ki");
            // ---- doubles: (V.T) pair matrices (eom_ccsd.py:352-372) --------------------------------------------------------
            M_C = keep(ov2);
            M_D = keep(ov2);
            M1 = keep(ov2);
            Ud = keep(ov2);
            M2 = keep(ov2);
            M12 = keep(ov2);
            MDU = keep(ov2);
            const TView Tdv = mv(Td, {v, o, v, o}), Txv = mv(Tx, {v, o, v, o});
            {
                // M1 = Wd' + 2 M_A - M_B with M_A = sum_kc V[k,l,c,d] T[c,a,k,i], M_B = sum_kc V[k,l,c,d] T[a,c,k,i]: the two share
                // their right operand, so the left ones are combined first — ONE (ov)^3 product instead of two
                Tmp TAB(*this, ov2);
                q.P(2.0, Tdv, "ckai", 0.0, mv(TAB, {v, o, v, o}), "aick");       // 2 T[c,a,k,i] - T[a,c,k,i] as [(a,i),(c,k)]
                q.P(-1.0, Txv, "aick", 1.0, mv(TAB, {v, o, v, o}), "aick");
                q.P(1.0, Viabj, "kaci", 0.0, mv(M1, {v, o, v, o}), "aick");      // Wd'[(a,i),(c,k)] = V_iabj[k,a,c,i]
                q.C(1.0, mv(TAB, {v, o, v, o}), "aick", mv(Vd, {v, o, v, o}), "ckdl", 1.0, mv(M1, {v, o, v, o}), "aidl");
                q.C(1.0, Tdv, "ckai", mv(Vx, {v, o, v, o}), "dlck", 0.0, mv(M_C, {v, o, v, o}), "aidl");   // sum_kc V[k,l,d,c] T[c,a,k,i]
                q.C(1.0, Txv, "aick", mv(Vx, {v, o, v, o}), "dlck", 0.0, mv(M_D, {v, o, v, o}), "aidl");   // sum_kc V[k,l,d,c] T[a,c,k,i]
            }
            q.P(1.0, Viajb, "kaic", 0.0, mv(Ud, {v, o, v, o}), "aick");          // Ud[(a,i),(c,k)] = V_iajb[k,a,i,c]
            q.L(M2, {M_D, M_C, Ud}, {1.0, -2.0, -1.0}, ov2);
            // exchange-symmetric trial doubles: M1.utd + M2.u2d + M_C.u2x = (2 M1 + M2).utd / 2 + (M_D - Ud).u2x / 2
            q.L(M12, {M1, M2}, {2.0, 1.0}, ov2);
            q.L(MDU, {M_D, Ud}, {1.0, -1.0}, ov2);
        }
        // V_kacd.T products of the u1 terms (eom_ccsd.py:334, :343, :345, :346), u-independent like the pair matrices above:
        //   WA[a,d,b,j] = sum_ck (2 V[k,a,c,d] - V[k,a,d,c]) T[c,b,k,j] - V[k,a,c,d] T[b,c,k,j],   W3[a,d,b,i] = sum_ck V[k,a,d,c] T[b,c,k,i]
        WA = keep(v * v * v * o);
        W3 = keep(v * v * v * o);
        {
            // (the first two terms share T[c,b,k,j]: 2 V[k,a,c,d] - V[k,a,d,c] is formed once — one o v^3 (ov) product less)
            Tmp Vt(*this, o * v * v * v);
            const TView VtV = mv(Vt, {o, v, v, v});
            q.P(2.0, Viabc, "kacd", 0.0, VtV, "kacd");
            q.P(-1.0, Viabc, "kadc", 1.0, VtV, "kacd");
            q.C(1.0, VtV, "kacd", T4, "cbkj", 0.0, mv(WA, {v, v, v, o}), "adbj");
        }
        q.C(-1.0, Viabc, "kacd", T4, "bckj", 1.0, mv(WA, {v, v, v, o}), "adbj");
        q.C(1.0, Viabc, "kadc", T4, "bcki", 0.0, mv(W3, {v, v, v, o}), "adbi");
        // ... merged: everything added to D is symmetrised by P(ijab,jiba) afterwards (:377), so a term X_abij may be replaced by
        // its partner X_baji — sum_d WA[a,d,b,j] u1[d,i] by sum_d WA[b,d,a,i] u1[d,j] — and the two terms become ONE product with
        // the free index of u1 innermost, WW[a,b,i,d] = WA[b,d,a,i] - W3[a,d,b,i]: [(a,b,i) x d] . u1[d,j] writes D in place, one
        // pass over one v^3 o array per build instead of two
        WW = keep(v * v * v * o);
        q.P(1.0, mv(WA, {v, v, v, o}), "bdai", 0.0, mv(WW, {v, v, o, v}), "abid");
        q.P(-1.0, mv(W3, {v, v, v, o}), "adbi", 1.0, mv(WW, {v, v, o, v}), "abid");
        // ... and the plain V_abic . u1 term (:349) has the same shape, [(a,b,i) x c] . u1[c,j]: it rides in the same product
        q.P(1.0, V("abic"), "abic", 1.0, mv(WW, {v, v, o, v}), "abic");
        for (double** w : {&WA, &W3}) {           // only WW is read by the builds
            owned_.erase(std::find(owned_.begin(), owned_.end(), *w));
            put(*w);
            *w = nullptr;
        }
        // The u2 parts of the one-index dressings (:353-354, :359-360) for an exchange-symmetric u2, whose crossed pair matrix
        // X[(a,j),(b,i)] = u2[a,b,i,j] is symmetric: both index placements of u2 are rows / columns of X itself,
        //   X_vv[a,c] = sum_kdl X[(a,k),(d,l)] (-2 V[l,k,c,d] + V[k,l,c,d]),   X_oo[k,i] = sum_dlc (-2 V[k,l,d,c] + V[k,l,c,d]) X[(d,l),(c,i)]
        // — ONE product each, X read in place, against two products over transposed copies before (2.2 ms of a 26-ms build of
        // four vectors at (30,120), rocprofv3 round 5)
        // (Bvv = columns [0, v) of BB[(k,d,l), v + o]; columns [v, v + o) hold the singles term :297 in the same form: with
        // Tt[(a,j),(b,k)] = 2 X[(a,k),(b,j)] - X[(a,j),(b,k)],  -sum_jbk Tt[(a,j),(b,k)] V[j,k,i,b] = sum_kbj X[(a,k),(b,j)] Bs[k,b,j,i],
        // Bs = -2 V[j,k,i,b] + V[k,j,i,b] — the stacked build gets X_vv AND that singles term from ONE pass over X)
        BB = keep(o * v * o * (v + o));
        {
            const TView BBv = mv(BB, {o, v, o, v + o});
            q.P(-2.0, Vijab, "lkcd", 0.0, slice(BBv, 3, 0, v), "kdlc");
            q.P(1.0, Vijab, "klcd", 1.0, slice(BBv, 3, 0, v), "kdlc");
            q.P(-2.0, Vijka, "jkib", 0.0, slice(BBv, 3, v, v + o), "kbji");
            q.P(1.0, Vijka, "kjib", 1.0, slice(BBv, 3, v, v + o), "kbji");
        }
        Aoo = keep(o * v * o * v);
        q.P(-2.0, Vijab, "kldc", 0.0, mv(Aoo, {o, v, o, v}), "kdlc");
        q.P(1.0, Vijab, "klcd", 1.0, mv(Aoo, {o, v, o, v}), "kdlc");
        // small hoisted V.T blocks
        A3 = keep(o * o * v * o);
        q.C(-2.0, Vijak, "klci", T4, "cbkj", 0.0, mv(A3, {o, o, v, o}), "libj");      // A_oovo
        q.C(1.0, Vijka, "klic", T4, "cbkj", 1.0, mv(A3, {o, o, v, o}), "libj");
        q.C(1.0, Vijak, "kldi", T4, "bdkj", 1.0, mv(A3, {o, o, v, o}), "libj");
        A4 = keep(o * o * v * o);
        q.C(1.0, Vijka, "klid", T4, "adkj", 0.0, mv(A4, {o, o, v, o}), "liaj");
        A6 = keep(o * v * o * o);
        q.C(1.0, Viabc, "lacd", T4, "cdji", 0.0, mv(A6, {o, v, o, o}), "laji");
        Gvv = keep(v * v);
        q.L(Gvv, {fvv}, {1.0}, v * v);
        q.C(-2.0, Vijab, "klcd", T4, "cakl", 1.0, mv(Gvv, {v, v}), "ad");
        q.C(1.0, Vijab, "klcd", T4, "ackl", 1.0, mv(Gvv, {v, v}), "ad");
        Goo = keep(o * o);
        q.L(Goo, {foo}, {-1.0}, o * o);
        q.C(-2.0, Vijab, "klcd", T4, "cdki", 1.0, mv(Goo, {o, o}), "li");
        q.C(1.0, Vijab, "kldc", T4, "cdki", 1.0, mv(Goo, {o, o}), "li");
        B2 = keep(o * o * o * o);
        q.P(1.0, Vklij, "klij", 0.0, mv(B2, {o, o, o, o}), "klij");
        q.C(1.0, Vijab, "klcd", T4, "cdij", 1.0, mv(B2, {o, o, o, o}), "klij");
        // particle ladder (:383): pair-packed form (1/4 of the flops) whenever V_abcd = V_badc and the trial doubles are
        // exchange-symmetric — true for every vector the Davidson driver generates
        v_sym = exchange_symmetric(Vabcd.p, v, v);
        // T_abij = T_baji (every CCSD solution): P(ijab,jiba)[T B5] = T (B5 + B5^(lkji)), so that term rides in the product
        // with B' of eom_ccsd.py:381 — one v^2 o^4 product less per sigma
        fused_ok = dev::fused_pair_kernels_ok(no);
        t_sym = exchange_symmetric(T, v, o);
        // eom_ccsd.py:380-382 in pair-packed rows needs B2_klij = B2_lkji and V_klcd = V_lkdc
        hole_sym = t_sym && exchange_symmetric(B2, o, o) && exchange_symmetric(Vijab.p, o, v);
        if (v_sym) L = keep(v * (v + 1) / 2 * o * o);
        many_ok = v_sym && hole_sym && fused_ok && t_sym;
        if (many_ok) {
            fovT = upload(0, o, o, v, 1.0, true);
            // the four u1 terms with one free index on u1 (A_oovo, A4, A6, V_iajk) as ONE product u1[a,l] A346[l,b,i,j]:
            // everything added to D is symmetrised by P(ijab,jiba) afterwards (:377), so a term X_abij may be replaced by its
            // partner X_baji
            A346 = keep(o * v * o * o);
            q.P(1.0, mv(A3, {o, o, v, o}), "libj", 0.0, mv(A346, {o, v, o, o}), "lbij");
            q.P(1.0, mv(A4, {o, o, v, o}), "ljbi", 1.0, mv(A346, {o, v, o, o}), "lbij");
            q.L(A346, {A346, A6, Viajk.p}, {1.0, -1.0, -1.0}, o * v * o * o);
            // ... and that product shares its shape with X_vv . T (:360-361): [z a] x (c | l) against the rows of T and of A346
            // stacked, TA[(c | l), (b,i,j)] — ONE product writes D (two passes over the k amplitude-sized accumulators before)
            TA = keep((v + o) * v * o * o);
            dev::memcpy_d2d(TA, T, sizeof(double) * v * v * o * o, e.stream);
            dev::memcpy_d2d(TA + v * v * o * o, A346, sizeof(double) * o * v * o * o, e.stream);
        }
    } catch (...) {
        for (double* p : owned_) e.scratch_put(p);
        owned_.clear();
        throw;
    }
}

// ---- eom_ccsd.py:268-310 -------------------------------------------------------------------------------------------------------
void EomSigma::singles(const double* u1, const double* u2, double* s1) {
    const int64_t o = no, v = nv;
    const Ops q{e};
    const TView U1 = mv(u1, {v, o}), U2 = mv(u2, {v, v, o, o}), S = mv(s1, {v, o});
    Tmp ut(*this, v * v * o * o);                                      // 2 u2[a,b,i,j] - u2[b,a,i,j]
    const TView Ut = mv(ut, {v, v, o, o});
    q.P(2.0, U2, "abij", 0.0, Ut, "abij");
    q.P(-1.0, U2, "baij", 1.0, Ut, "abij");
    q.C(1.0, U1, "ck", mv(W1, {v, o, v, o}), "ckai", 0.0, S, "ai");
    q.C(1.0, mv(Gvv_s, {v, v}), "ac", U1, "ci", 1.0, S, "ai");
    q.C(1.0, U1, "ak", mv(Goo_s, {o, o}), "ki", 1.0, S, "ai");
    q.C(1.0, mv(fov, {o, v}), "jb", Ut, "baji", 1.0, S, "ai");
    q.C(-1.0, V("ijka"), "jkib", Ut, "abjk", 1.0, S, "ai");
    q.C(1.0, V("iabc"), "jabc", Ut, "bcji", 1.0, S, "ai");
}

// ---- eom_ccsd.py:312-385 -------------------------------------------------------------------------------------------------------
void EomSigma::doubles(const double* u1, const double* u2, bool u2_sym, double* s2, bool defer_ladder) {
    const int64_t o = no, v = nv, ov = o * v, ov2 = ov * ov, npp = v * (v + 1) / 2;
    const Ops q{e};
    const TView U1 = mv(u1, {v, o}), U2 = mv(u2, {v, v, o, o}), T4 = mv(T, {v, v, o, o});
    const TView Vijab = V("ijab"), Vijka = V("ijka"), Vijak = V("ijak"), Viabc = V("iabc");
    auto P4 = [&](double* p) { return mv(p, {v, o, v, o}); };
    // a trial vector without exchange symmetry: the five (ov)^3 products as TWO, stacked along the summed pair index
    const bool kstack = !u2_sym && fused_ok;
    Tmp u2x(*this, kstack ? 1 : ov2), utd(*this, kstack ? 1 : ov2), Dx(*this, ov2), Dd(*this, ov2);
    Tmp u2d(*this, u2_sym || kstack ? 1 : ov2), R3(*this, kstack ? 3 * ov2 : 1);
    // the pair layouts u2x[(a,j),(b,i)] = u2[a,b,i,j], utd = 2 u2d - (u2[b,a,i,j] in the u2d layout), u2d[(a,i),(b,j)] = u2[a,b,i,j]
    if (kstack) {
        // R3 = [u2d ; u2x^T ; u2x] from one pass over u2 (u2x^T[(d,l),(b,j)] = u2[b,d,l,j] is "u2[b,a,i,j] in the u2d layout"):
        //   Dd = M1.(2 u2d - u2x^T) + M2.u2d + M_C.u2x = [2 M1 + M2 | -M1 | M_C] . R3                       (K = 3 ov)
        //   Dx = M_D.u2x - u2x.Ud^T, and since only Dx + Dx^T enters (:377, the assembly below) the second term may be
        //   transposed: Dx' = [-Ud | M_D] . [u2x^T ; u2x]                                                      (K = 2 ov)
        // same flops, but 841 tiles x 5 launches with their cut tails become two long launches (8.0 -> 6.9 ms at (30,120))
        general_operands();
        dev::t2_layouts(u2, R3.p, R3.p + 2 * ov2, R3.p + ov2, no, nv, e.stream, 0.0, 1.0);
        q.C(1.0, mv(LK3, {v, o, 3, v, o}), "aisdl", mv(R3.p, {3, v, o, v, o}), "sdlbj", 0.0, P4(Dd), "aibj");
        q.C(1.0, mv(LK2, {v, o, 2, v, o}), "ajsdl", mv(R3.p + ov2, {2, v, o, v, o}), "sdlbi", 0.0, P4(Dx), "ajbi");
    } else if (fused_ok) {             // ... in ONE pass over u2 (the kernel of the CCSD residual's layouts)
        dev::t2_layouts(u2, u2_sym ? nullptr : u2d.p, u2x, utd, no, nv, e.stream);
    } else {
        q.P(1.0, U2, "abij", 0.0, P4(u2x), "ajbi");
        q.P(2.0, U2, "abij", 0.0, P4(utd), "aibj");                     // ut[d,b,l,j] = 2u2[d,b,l,j] - u2[b,d,l,j]
        q.P(-1.0, U2, "baij", 1.0, P4(utd), "aibj");
        if (!u2_sym) q.P(1.0, U2, "abij", 0.0, P4(u2d), "aibj");
    }
    // ---- (ov)^3 products ---------------------------------------------------------------------------------------------------
    if (u2_sym) {
        // exchange-symmetric u2: utd = 2 u2d - u2x as matrices, hence M1.utd + M2.u2d + M_C.u2x = (2 M1 + M2).utd / 2 +
        // (M_D - Ud).u2x / 2, and the second product IS Dx (the C / D form of the ring terms): TWO (ov)^3 products per sigma
        q.C(1.0, P4(MDU), "ajdl", P4(u2x), "dlbi", 0.0, P4(Dx), "ajbi");                       // :372 and :364 (transposed)
        // Dd also carries Dx / 2 in the direct placement: the fused assembly reads Dx there itself (xd), else a scaled copy
        if (!fused_ok) q.P(0.5, P4(Dx), "ajbi", 0.0, P4(Dd), "ajbi");                          // same memory layout as "aibj"
        q.C(0.5, P4(M12), "aidl", P4(utd), "dlbj", fused_ok ? 0.0 : 1.0, P4(Dd), "aibj");
    } else if (!kstack) {
        q.C(1.0, P4(M1), "aidl", P4(utd), "dlbj", 0.0, P4(Dd), "aibj");
        q.C(1.0, P4(M2), "aidl", P4(u2d), "dlbj", 1.0, P4(Dd), "aibj");
        q.C(1.0, P4(M_C), "aidl", P4(u2x), "dlbj", 1.0, P4(Dd), "aibj");                      // u2x[(d,l),(b,j)] = u2[d,b,j,l]
        q.C(1.0, P4(M_D), "ajdl", P4(u2x), "dlbi", 0.0, P4(Dx), "ajbi");                      // :372  u2[d,b,i,l]
        q.C(-1.0, P4(u2x), "ajck", P4(Ud), "bick", 1.0, P4(Dx), "ajbi");                      // :364
    }
    // ---- one-index dressings ---------------------------------------------------------------------------------------------------
    Tmp Xoo(*this, o * o), Xvv(*this, v * v), B5(*this, o * o * o * o);
    const TView XooV = mv(Xoo, {o, o}), XvvV = mv(Xvv, {v, v}), FOV = mv(fov, {o, v});
    q.C(-2.0, Vijka, "klid", U1, "dl", 0.0, XooV, "ki");
    q.C(1.0, Vijak, "kldi", U1, "dl", 1.0, XooV, "ki");
    q.C(-1.0, FOV, "kd", U1, "di", 1.0, XooV, "ki");
    if (u2_sym) {
        q.C(1.0, mv(Aoo, {o, v, o, v}), "kdlc", P4(u2x), "dlci", 1.0, XooV, "ki");
    } else {
        q.C(-2.0, Vijab, "kldc", U2, "dcil", 1.0, XooV, "ki");
        q.C(1.0, Vijab, "kldc", U2, "dcli", 1.0, XooV, "ki");
    }
    q.C(1.0, XooV, "ki", P4(Td), "akbj", 1.0, P4(Dd), "aibj", "a");
    q.C(2.0, Viabc, "ladc", U1, "dl", 0.0, XvvV, "ac");
    q.C(-1.0, Viabc, "lacd", U1, "dl", 1.0, XvvV, "ac");
    q.C(-1.0, U1, "al", FOV, "lc", 1.0, XvvV, "ac");
    if (u2_sym) {
        q.C(1.0, P4(u2x), "akdl", slice(mv(BB, {o, v, o, v + o}), 3, 0, v), "kdlc", 1.0, XvvV, "ac");
    } else {
        q.C(-2.0, Vijab, "lkcd", U2, "adlk", 1.0, XvvV, "ac");
        q.C(1.0, Vijab, "lkcd", U2, "dalk", 1.0, XvvV, "ac");
    }
    const bool packed = v_sym && u2_sym && hole_sym;
    const bool fused = packed && fused_ok;
    // D goes straight into the caller's array unless the fused assembly needs it as an input
    Tmp Dtmp(*this, fused_ok ? v * v * o * o : 1);
    double* Dp = fused_ok ? Dtmp.p : s2;
    TView D = mv(Dp, {v, v, o, o});
    q.C(1.0, XvvV, "ac", T4, "cbij", 0.0, D, "abij");
    // V_kacd.T.u1 terms (:334, :343, :345, :346) through the hoisted V.T intermediates: o^2 v^3 instead of (ov)^3 each
    q.C(1.0, mv(WW, {v, v, o, v}), "abid", U1, "dj", 1.0, D, "abij");
    q.C(1.0, mv(Gvv, {v, v}), "ad", U2, "dbij", 1.0, D, "abij");
    q.C(1.0, mv(Goo, {o, o}), "li", U2, "ablj", 1.0, D, "abij", "ab");
    q.C(1.0, U1, "al", mv(A3, {o, o, v, o}), "libj", 1.0, D, "abij");
    q.C(1.0, U1, "bl", mv(A4, {o, o, v, o}), "liaj", 1.0, D, "abij");
    q.C(-1.0, U1, "bl", mv(A6, {o, v, o, o}), "laji", 1.0, D, "abij");
    const TView B5v = mv(B5, {o, o, o, o});
    q.C(1.0, Vijka, "klid", U1, "dj", 0.0, B5v, "klij");
    if (!t_sym) q.C(1.0, T4, "abkl", B5v, "klij", 1.0, D, "abij");
    q.C(-1.0, U1, "ak", V("iajk"), "kbij", 1.0, D, "abij");
    auto packed_terms = [&]() {       // the terms (:380-383) that stay outside P(ijab,jiba), in the pair-packed rows L
        Tmp B5s(*this, o * o * o * o);
        q.P(1.0, B5v, "klij", 0.0, mv(B5s, {o, o, o, o}), "klij");
        q.P(1.0, B5v, "lkji", 1.0, mv(B5s, {o, o, o, o}), "klij");
        e.ladder_sym(u2, L, 0, npp, dressed, 0);
        e.hole_ladder_packed(u2, B2, L, 0, npp, nullptr);
        e.hole_ladder_packed(T, B5s, L, 0, npp, u2);
    };
    if (fused) {
        // symmetrisation (:377) of D and of the two pair matrices and the unpacking of L in ONE pass (the assembly kernel of
        // the CCSD residual)
        packed_terms();
        dev::residual_assemble(nullptr, L, Dp, Dd, Dx, s2, no, nv, e.stream, 0.5);
        return;
    }
    // ---- P(ijab, jiba) (:377), then the unpermuted terms (:380-383) ------------------------------------------------------------
    if (fused_ok) {                    // D + P D and the two pair matrices with their transposes in one pass, into the result
        dev::residual_assemble(nullptr, nullptr, Dp, Dd, Dx, s2, no, nv, e.stream, u2_sym ? 0.5 : 0.0);
        Dp = s2;
        D = mv(Dp, {v, v, o, o});
    } else {
        q.P(1.0, P4(Dd), "aibj", 1.0, D, "abij");
        q.P(1.0, P4(Dx), "ajbi", 1.0, D, "abij");
        Tmp S(*this, v * v * o * o);
        q.P(1.0, D, "baji", 0.0, mv(S, {v, v, o, o}), "abij");
        q.L(Dp, {Dp, S}, {1.0, 1.0}, v * v * o * o);
    }
    if (packed) {
        packed_terms();
        e.ladder_sym_unpack(L, Dp, 1.0);
        return;
    }
    Tmp Bn(*this, o * o * o * o);
    const TView BnV = mv(Bn, {o, o, o, o});
    q.C(1.0, Vijab, "kldc", U2, "dcij", 0.0, BnV, "klij");
    if (t_sym) {                       // + the symmetrised u1 term that was held back above
        q.P(1.0, B5v, "klij", 1.0, BnV, "klij");
        q.P(1.0, B5v, "lkji", 1.0, BnV, "klij");
    }
    q.C(1.0, U2, "abkl", mv(B2, {o, o, o, o}), "klij", 1.0, D, "abij");               // :380, :382
    q.C(1.0, T4, "abkl", BnV, "klij", 1.0, D, "abij");                                  // :381
    if (v_sym && u2_sym) {                                                              // :383
        e.ladder_sym(u2, L, 0, npp, dressed, 0);
        e.ladder_sym_unpack(L, Dp, 1.0);
    } else if (v_sym) {
        if (!defer_ladder) {
            const double* us[1] = {u2};
            double* ss[1] = {Dp};
            general_ladders(1, us, ss);
        }
    } else {
        q.C(1.0, V("abcd"), "abcd", U2, "cdij", 1.0, D, "abij");
    }
}

// The u-independent left operands of the two stacked (ov)^3 products of doubles() for a trial vector without exchange symmetry
void EomSigma::general_operands() {
    if (LK3) return;
    const int64_t ov = static_cast<int64_t>(no) * nv;
    const Ops q{e};
    LK3 = keep(3 * ov * ov);
    LK2 = keep(2 * ov * ov);
    auto columns = [&](double* dst, int64_t width, int64_t s, double c0, const double* m0, double c1, const double* m1) {
        const int64_t dims[2] = {ov, ov}, st[2] = {width * ov, 1};
        const TView out = make_view(dst + s * ov, 2, dims, st);
        q.P(c0, mv(m0, {ov, ov}), "xy", 0.0, out, "xy");
        if (m1) q.P(c1, mv(m1, {ov, ov}), "xy", 1.0, out, "xy");
    };
    columns(LK3, 3, 0, 2.0, M1, 1.0, M2);
    columns(LK3, 3, 1, -1.0, M1, 0.0, nullptr);
    columns(LK3, 3, 2, 1.0, M_C, 0.0, nullptr);
    columns(LK2, 2, 0, -1.0, Ud, 0.0, nullptr);
    columns(LK2, 2, 1, 1.0, M_D, 0.0, nullptr);
}

// The particle ladder (:383) of g trial vectors WITHOUT exchange symmetry, added to s2[z].  It acts on (i,j) as spectators and
// commutes with the exchange P (V_abcd = V_badc): with u = us + ua (us = (u + P u) / 2) the symmetric part runs pair-packed as
// it stands, and so does the antisymmetric one after w_abij = sgn(i - j) ua_abij (exchange-symmetric, zero for i == j):
// Lad(ua)_abij = sgn(i - j) Lad(w)_abij; the o columns i == j that w leaves out are a skinny plain product.  2 g quarter-flop
// ladders in ONE batched launch per half (the packed integrals read once) + v^4 o flops per vector instead of g full v^4 o^2
// products.  (Nothing else of the general build can be split this way: the reference's symmetrised part is not P-covariant,
// DESIGN 6e.)
void EomSigma::general_ladders(int g, const double* const* u2, double* const* s2) {
    const int64_t o = no, v = nv, n2 = v * v * o * o, npp = v * (v + 1) / 2, G = g;
    const Ops q{e};
    Tmp usw(*this, 2 * G * n2), dg(*this, G * v * v * o), Lall(*this, 2 * G * npp * o * o), R2(*this, n2), Rd(*this, G * v * v * o);
    std::vector<const double*> xs(2 * g);
    for (int z = 0; z < g; ++z) {
        double *us = usw.p + 2 * z * n2, *w = us + n2;
        dev::exchange_split(u2[z], us, w, dg.p + z * v * v * o, no, nv, e.stream);
        xs[2 * z] = us;
        xs[2 * z + 1] = w;
    }
    e.ladder_sym_multi(xs.data(), 2 * g, Lall, dressed);
    // the diagonal columns of all vectors from one pass over V_abcd
    q.C(1.0, V("abcd"), "abcd", mv(dg, {G, v, v, o}), "zcdi", 0.0, mv(Rd, {G, v, v, o}), "zabi");
    for (int z = 0; z < g; ++z) {
        e.ladder_sym_unpack(Lall.p + 2 * z * npp * o * o, s2[z], 1.0);
        e.ladder_sym_unpack(Lall.p + (2 * z + 1) * npp * o * o, R2, 0.0);
        dev::sgn_ij_add(s2[z], R2, no, nv, e.stream);
        const int64_t dims[3] = {v, v, o}, st[3] = {v * o * o, o * o, o + 1};
        q.P(1.0, mv(Rd.p + z * v * v * o, {v, v, o}), "abi", 1.0, make_view(s2[z], 3, dims, st), "abi");      // s2[a,b,i,i] += Rd[a,b,i]
    }
}

int EomSigma::stack_limit() const {
    // nine (ov)^2-sized temporaries per vector (X, Tt, DxT, DdT, D, the packed ladder rows and their operands) must fit in
    // half of what the device has free right now (pooled buffers count as free)
    const double free_b = static_cast<double>(dev::mem_free_bytes()) + static_cast<double>(e.scratch_free_bytes());
    const double per_vector = 9.0 * 8.0 * static_cast<double>(no) * nv * static_cast<double>(no) * nv;
    return static_cast<int>(std::max(1.0, std::min(16.0, std::floor(free_b / 2.0 / std::max(per_vector, 1.0)))));
}

// ---- sigma for k exchange-symmetric trial vectors at once: every operand that does not depend on the vector is read ONCE ----
void EomSigma::stack(int k, const double* const* u1, const double* const* u2, double* const* s1, double* const* s2) {
    const int64_t o = no, v = nv, ov = o * v, ov2 = ov * ov, npp = v * (v + 1) / 2, K = k;
    const Ops q{e};
    const TView Vijka = V("ijka"), Vijak = V("ijak"), Viabc = V("iabc");
    Tmp U1(*this, K * v * o), X(*this, K * ov2), Tt(*this, K * ov2);
    for (int z = 0; z < k; ++z) {
        dev::memcpy_d2d(U1.p + z * v * o, u1[z], sizeof(double) * v * o, e.stream);
        // X[z,(a,j),(b,i)] = u2_z[a,b,i,j], Tt[z,(a,i),(b,j)] = 2 u2_z[a,b,i,j] - u2_z[b,a,i,j]        (symmetric matrices)
        dev::t2_layouts(u2[z], nullptr, X.p + z * ov2, Tt.p + z * ov2, no, nv, e.stream);
    }
    const TView U1v = mv(U1, {K, v, o}), Xv = mv(X, {K, v, o, v, o}), Ttv = mv(Tt, {K, v, o, v, o});
    // ---- singles (eom_ccsd.py:268-310), ut[a,b,i,j] = Tt[(a,i),(b,j)] -----------------------------------------------------------
    Tmp S1(*this, K * v * o);
    const TView S1v = mv(S1, {K, v, o});
    q.C(1.0, U1v, "zck", mv(W1, {v, o, v, o}), "ckai", 0.0, S1v, "zai");
    q.C(1.0, mv(Gvv_s, {v, v}), "ac", U1v, "zci", 1.0, S1v, "zai", "z");
    q.C(1.0, U1v, "zak", mv(Goo_s, {o, o}), "ki", 1.0, S1v, "zai");
    q.C(1.0, Ttv, "zaibj", mv(fovT, {v, o}), "bj", 1.0, S1v, "zai");
    // X_vv's u2 part (:359-360) and the singles term :297 from one pass over X: XS[z,a,:] = X[z,(a,k),(d,l)] BB[(k,d,l),:]
    Tmp XS(*this, K * v * (v + o));
    const TView XSv = mv(XS, {K, v, v + o});
    q.C(1.0, Xv, "zakdl", mv(BB, {o, v, o, v + o}), "kdln", 0.0, XSv, "zan");
    e.axpby(1.0, slice(XSv, 2, v, v + o), 1.0, S1v);
    q.C(1.0, Viabc, "jabc", Ttv, "zbjci", 1.0, S1v, "zai", "z");                       // (z as a batch: Tt is read in place)
    // ---- (ov)^3 products, transposed: only Dx + Dx^T and Dd + Dd^T enter (:377), X and Tt are symmetric matrices ---------------
    Tmp DxT(*this, K * ov2), DdT(*this, K * ov2);
    const TView DxTv = mv(DxT, {K, v, o, v, o}), DdTv = mv(DdT, {K, v, o, v, o});
    q.C(1.0, Xv, "zajdl", mv(MDU, {v, o, v, o}), "bidl", 0.0, DxTv, "zajbi");          // (MDU . u2x)^T per vector
    // (DdT also carries DxT / 2 in the direct placement: the assembly below reads DxT there itself, xd = 0.5 — no scaled copy)
    q.C(0.5, Ttv, "zaidl", mv(M12, {v, o, v, o}), "bjdl", 0.0, DdTv, "zaibj");
    // ---- one-index dressings -------------------------------------------------------------------------------------------------------
    Tmp Xoo(*this, K * o * o), Xvv(*this, K * v * v);
    const TView XooV = mv(Xoo, {K, o, o}), XvvV = mv(Xvv, {K, v, v}), FOV = mv(fov, {o, v});
    q.C(-2.0, Vijka, "klid", U1v, "zdl", 0.0, XooV, "zki");
    q.C(1.0, Vijak, "kldi", U1v, "zdl", 1.0, XooV, "zki");
    q.C(-1.0, FOV, "kd", U1v, "zdi", 1.0, XooV, "zki", "z");
    q.C(1.0, mv(Aoo, {o, v, o, v}), "kdlc", Xv, "zdlci", 1.0, XooV, "zki", "z");       // u2[d,c,i,l] = X[(d,l),(c,i)], both placements
    q.C(1.0, XooV, "zki", mv(Td, {v, o, v, o}), "akbj", 1.0, DdTv, "zaibj", "za");
    q.C(2.0, Viabc, "ladc", U1v, "zdl", 0.0, XvvV, "zac");
    q.C(-1.0, Viabc, "lacd", U1v, "zdl", 1.0, XvvV, "zac");
    q.C(-1.0, U1v, "zal", FOV, "lc", 1.0, XvvV, "zac");
    e.axpby(1.0, slice(XSv, 2, 0, v), 1.0, XvvV);                                       // u2[a,d,l,k] = X[(a,k),(d,l)], both placements
    Tmp D(*this, K * v * v * o * o);
    const TView Dv = mv(D, {K, v, v, o, o});
    {
        // D = [X_vv | u1] . [T ; A346]   (:360-361 and the four u1 terms with a free index on u1, see the hoist)
        Tmp XU(*this, K * v * (v + o));
        const TView XUv = mv(XU, {K, v, v + o});
        e.copy(XvvV, slice(XUv, 2, 0, v));
        e.copy(U1v, slice(XUv, 2, v, v + o));
        q.C(1.0, XUv, "zan", mv(TA, {v + o, v, o, o}), "nbij", 0.0, Dv, "zabij");
    }
    q.C(1.0, mv(WW, {v, v, o, v}), "abid", U1v, "zdj", 1.0, Dv, "zabij", "z");
    Tmp Lall(*this, K * npp * o * o);
    e.ladder_sym_multi(u2, k, Lall, dressed);                                           // :383, all vectors
    Tmp B5(*this, K * o * o * o * o), B5s(*this, K * o * o * o * o);
    std::vector<const double*> b2s(k, B2), ts(k, T), b5p(k);
    for (int z = 0; z < k; ++z) {
        // (G_vv . u2, G_oo . u2 per vector: a batched launch over a stacked direct layout moves the same bytes — measured)
        const TView Dz = mv(D.p + z * v * v * o * o, {v, v, o, o}), U2z = mv(u2[z], {v, v, o, o});
        q.C(1.0, mv(Gvv, {v, v}), "ad", U2z, "dbij", 1.0, Dz, "abij");
        q.C(1.0, mv(Goo, {o, o}), "li", U2z, "ablj", 1.0, Dz, "abij", "ab");
        const TView B5z = mv(B5.p + z * o * o * o * o, {o, o, o, o}), B5sz = mv(B5s.p + z * o * o * o * o, {o, o, o, o});
        q.C(1.0, Vijka, "klid", mv(U1.p + z * v * o, {v, o}), "dj", 0.0, B5z, "klij");
        q.P(1.0, B5z, "klij", 0.0, B5sz, "klij");
        q.P(1.0, B5z, "lkji", 1.0, B5sz, "klij");
        b5p[z] = B5sz.p;
    }
    // the hole-ladder-shaped terms of all vectors in batched launches (the shared side — V_klij + V_klcd T_cdij, then T —
    // packed once)
    e.hole_ladder_packed_multi(u2, b2s.data(), nullptr, k, Lall);                      // :380, :382
    e.hole_ladder_packed_multi(ts.data(), b5p.data(), u2, k, Lall);                    // :381 (+ the symmetrised u1 term)
    for (int z = 0; z < k; ++z) {
        dev::residual_assemble(nullptr, Lall.p + z * npp * o * o, D.p + z * v * v * o * o, DdT.p + z * ov2, DxT.p + z * ov2, s2[z],
                               no, nv, e.stream, 0.5);                                  // :377 + unpacking
        dev::memcpy_d2d(s1[z], S1.p + z * v * o, sizeof(double) * v * o, e.stream);
    }
}

void EomSigma::apply(int k, const double* const* u1, const double* const* u2, const int* sym, double* const* s1,
                     double* const* s2) {
    if (k < 1) return;
    const int64_t o = no, v = nv;
    std::vector<int> sy(k);
    bool all = true;
    for (int z = 0; z < k; ++z) {
        if (!u1[z] || !u2[z] || !s1[z] || !s2[z]) throw Error("eom sigma: null vector");
        sy[z] = sym ? (sym[z] != 0) : exchange_symmetric(u2[z], v, o);
        all = all && sy[z];
    }
    auto one = [&](int z, bool defer = false) {
        singles(u1[z], u2[z], s1[z]);
        doubles(u1[z], u2[z], sy[z] != 0, s2[z], defer);
    };
    if (k < 2 || !many_ok || !all) {
        // vectors without exchange symmetry: their particle ladders are held back and run together, eight vectors at a time
        std::vector<const double*> gu;
        std::vector<double*> gs;
        for (int z = 0; z < k; ++z) {
            const bool defer = k > 1 && v_sym && !sy[z];
            one(z, defer);
            if (defer) {
                gu.push_back(u2[z]);
                gs.push_back(s2[z]);
            }
            if (gu.size() == 8 || (z == k - 1 && !gu.empty())) {
                general_ladders(static_cast<int>(gu.size()), gu.data(), gs.data());
                gu.clear();
                gs.clear();
            }
        }
        return;
    }
    const int step = stack_limit();
    for (int lo = 0; lo < k; lo += step) {
        const int hi = std::min(k, lo + step);
        if (hi - lo < 2) { one(lo); continue; }
        try {
            stack(hi - lo, u1 + lo, u2 + lo, s1 + lo, s2 + lo);
        } catch (const Error& err) {
            if (std::string(err.what()).find("memory") == std::string::npos) throw;
            trim();                    // out of device memory in the middle of a stacked build: one vector at a time
            for (int z = lo; z < hi; ++z) one(z);
        }
    }
}

// ==== the adjoint of the sigma build: left vectors, the Lambda equations, the one-particle density ====================
// apply() on an exchange-symmetric u2 is a chain of linear steps (the u2_sym branches of singles() / doubles()); A^T l runs that
// chain backwards with every product transposed — the same hoisted operands through transposed views, no new intermediate of
// V and T.  The steps under the permutation P(ijab,jiba) (:377) see l2 + l2^T = 2 l2, the unpermuted ones (:380-383) l2; the
// result is projected back onto the symmetric subspace by the assembly kernel.
//
// The partial results of A^T l for K >= 1 vectors — S1, D, Pd, Px stacked by vector, the packed ladder halves of the K vectors
// side by side in rows of pitch K ld (Engine::ladder_sym_adjoint_multi) — and what dev::lambda_assemble reads of them, one
// description per vector: the caller adds the coefficients, the outputs and, for a Lambda step, the operands of the update.
struct EomSigma::LeftBuild {
    const int64_t K, n1, n2;
    const PairDims pd;
    const bool la;                     // the antisymmetric ladder half exists
    Tmp S1, D, Pd, Px, Lp, La;
    std::vector<dev::LambdaParts> parts;
    LeftBuild(EomSigma& s, int k)
        : K(k), n1(static_cast<int64_t>(s.nv) * s.no), n2(n1 * n1), pd(s.no, s.nv), la(s.v_sym && s.no > 1 && s.nv > 1),
          S1(s, K * n1), D(s, K * n2), Pd(s, K * n2), Px(s, K * n2), Lp(s, s.v_sym ? pd.npp * K * pd.adj_ldp : 1),
          La(s, la ? pd.npm * K * pd.adj_ldm : 1), parts(static_cast<size_t>(k)) {
        for (int64_t z = 0; z < K; ++z) {
            dev::LambdaParts& q = parts[z];
            q.S1 = S1.p + z * n1; q.D = D.p + z * n2; q.Pd = Pd.p + z * n2; q.Px = Px.p + z * n2;
            if (s.v_sym) { q.Lp = Lp.p + z * pd.adj_ldp; q.lp_ld = K * pd.adj_ldp; }
            if (la) { q.La = La.p + z * pd.adj_ldm; q.la_ld = K * pd.adj_ldm; }
        }
    }
};

// The refusals of the left build that the shape alone decides: before anything is tested, hoisted or allocated
void EomSigma::left_check() const {
    if (!fused_ok) throw Error("eom sigma apply_left: nocc too large for the fused pair kernels");
    if (!dev::lambda_assemble_ok(no))
        throw Error("lambda_assemble: nocc = " + std::to_string(no) + " is too large for the LDS tile (o (o + 1) + 256 doubles in 64 KB: nocc <= " +
                    std::to_string(PYMES_NOCC_MAX_LAMBDA) + ")");
}

void EomSigma::left_prepare() {
    left_check();
    if (left_ready) return;
    const int64_t o = no, v = nv;
    const Ops q{e};
    if (!eta1) eta1 = keep(v * o);
    q.P(2.0, mv(fov, {o, v}), "ia", 0.0, mv(eta1, {v, o}), "ai");
    left_ready = true;
}

void EomSigma::apply_left(int k, const double* const* l1, const double* const* l2, const int* sym, double* const* o1,
                          double* const* o2) {
    if (k < 1) return;
    left_check();
    for (int z = 0; z < k; ++z)
        if (!l1[z] || !l2[z] || !o1[z] || !o2[z]) throw Error("eom sigma apply_left: null vector");
    for (int z = 0; z < k; ++z)            // (refusals first: nothing is allocated for a call that is refused)
        if (!(sym && sym[z]) && !exchange_symmetric(l2[z], nv, no))
            throw Error("eom sigma apply_left: the left doubles do not have the exchange symmetry l2_abij = l2_baji");
    left_prepare();
    auto build = [&](int lo, int hi) {
        LeftBuild w(*this, hi - lo);
        left_build(l1 + lo, l2 + lo, w);
        for (int z = lo; z < hi; ++z) {
            dev::LambdaParts& q = w.parts[z - lo];
            q.cd = 2.0; q.cx = -1.0;
            q.out1 = o1[z]; q.out2 = o2[z];
            dev::lambda_assemble(q, no, nv, e.stream);
        }
    };
    const int step = k > 1 ? stack_limit() : 1;
    for (int lo = 0; lo < k; lo += step) {
        const int hi = std::min(k, lo + step);
        try {
            build(lo, hi);
        } catch (const Error& err) {
            if (hi - lo < 2 || std::string(err.what()).find("memory") == std::string::npos) throw;
            trim();                    // out of device memory in the middle of a stacked build: one vector at a time
            for (int z = lo; z < hi; ++z) build(z, z + 1);
        }
    }
}

// ---- the partial results of A^T l for the K = w.K left vectors l1[z], l2[z]: every vector-dependent operand carries a leading
// vector index, so that every hoisted operand and every V+ / V- row is read once per call.  A stack of one is the caller's vector,
// read in place.  The two (ov)^3 products run transposed — PdT[z] = ld_z M12, PxT[z] = Q_z MDU with the K symmetric pair matrices
// stacked along the rows: ONE GEMM each — which the assembly does not see: it reads Pd and Px only through raw_abij + raw_baji,
// the sum of an element and its transpose.  For the same reason every term of Px may lie either way: the two small products that
// add into it are placed the way their GEMM writes them, without a copy for any K.  The packed ladder halves of the K vectors
// lie side by side in the columns of one product per half (Engine::ladder_sym_adjoint_multi).
void EomSigma::left_build(const double* const* l1, const double* const* l2, LeftBuild& w) {
    const int64_t o = no, v = nv, ov = o * v, ov2 = ov * ov, K = w.K, n1 = w.n1, n2 = w.n2;
    const int k = static_cast<int>(K);
    const Ops q{e};
    std::optional<Tmp> L1S, L2S;
    if (k > 1) {
        L1S.emplace(*this, K * n1);
        L2S.emplace(*this, K * n2);
    }
    const double *l1s = k > 1 ? L1S->p : l1[0], *l2s = k > 1 ? L2S->p : l2[0];
    // Pair layouts of l2 in one pass: ld[(a,i),(b,j)] = lx[(a,j),(b,i)] = l2_abij, and Q = ld + 2 lx as matrices — what Dx
    // receives: 2 lx where it enters D, ld / 2 . 2 through the half of it that Dd carries
    Tmp ld(*this, K * ov2), lx(*this, K * ov2), Q(*this, K * ov2);
    for (int z = 0; z < k; ++z) {
        if (k > 1) {
            dev::memcpy_d2d(L1S->p + z * n1, l1[z], sizeof(double) * n1, e.stream);
            dev::memcpy_d2d(L2S->p + z * n2, l2[z], sizeof(double) * n2, e.stream);
        }
        dev::t2_layouts(l2[z], ld.p + z * ov2, lx.p + z * ov2, Q.p + z * ov2, no, nv, e.stream, 1.0, 2.0);
    }
    const TView L1 = mv(l1s, {K, v, o}), L2 = mv(l2s, {K, v, v, o, o}), T4 = mv(T, {v, v, o, o});
    const TView Vijab = V("ijab"), Vijka = V("ijka"), Vijak = V("ijak"), Viabc = V("iabc");
    const TView S = mv(w.S1, {K, v, o}), D = mv(w.D, {K, v, v, o, o}), FOV = mv(fov, {o, v});
    auto P4 = [&](const double* p) { return mv(p, {v, o, v, o}); };
    auto P5 = [&](const double* p) { return mv(p, {K, v, o, v, o}); };
    // ---- singles() backwards: the l1 row of A^T ------------------------------------------------------------------------------------
    q.C(1.0, mv(W1, {v, o, v, o}), "ckai", L1, "zai", 0.0, S, "zck");
    q.C(1.0, mv(Gvv_s, {v, v}), "ac", L1, "zai", 1.0, S, "zci");
    q.C(1.0, L1, "zai", mv(Goo_s, {o, o}), "ki", 1.0, S, "zak");
    {
        // the adjoint of ut = 2 u2 - u2^(ab): utb collects what singles() contracts ut with, then D = 2 utb - utb^(ab)
        Tmp utb(*this, K * n2);
        const TView Ub = mv(utb, {K, v, v, o, o});
        q.C(1.0, mv(fov, {o, v, 1}), "jbx", mv(l1s, {K, 1, v, o}), "zxai", 0.0, Ub, "zbaji");   // (an outer product: K = 1)
        q.C(-1.0, Vijka, "jkib", L1, "zai", 1.0, Ub, "zabjk");
        q.C(1.0, Viabc, "jabc", L1, "zai", 1.0, Ub, "zbcji");
        q.P(2.0, Ub, "zabij", 0.0, D, "zabij");
        q.P(-1.0, Ub, "zbaij", 1.0, D, "zabij");
    }
    // ---- doubles() backwards ---------------------------------------------------------------------------------------------------------
    Tmp Xoo(*this, K * o * o), Xvv(*this, K * v * v), Bn(*this, K * o * o * o * o);
    const TView XooV = mv(Xoo, {K, o, o}), XvvV = mv(Xvv, {K, v, v}), BnV = mv(Bn, {K, o, o, o, o});
    // the terms that wrote D (:334-361): their operand against 2 l2
    q.C(2.0, L2, "zabij", T4, "cbij", 0.0, XvvV, "zac");
    q.C(2.0, mv(WW, {v, v, o, v}), "abid", L2, "zabij", 1.0, S, "zdj");
    q.C(2.0, mv(Gvv, {v, v}), "ad", L2, "zabij", 1.0, D, "zdbij", "z");
    q.C(2.0, mv(Goo, {o, o}), "li", L2, "zabij", 1.0, D, "zablj", "zab");
    q.C(2.0, L2, "zabij", mv(A3, {o, o, v, o}), "libj", 1.0, S, "zal");
    q.C(2.0, L2, "zabij", mv(A4, {o, o, v, o}), "liaj", 1.0, S, "zbl");
    q.C(-2.0, L2, "zabij", mv(A6, {o, v, o, o}), "laji", 1.0, S, "zbl");
    q.C(-2.0, L2, "zabij", V("iajk"), "kbij", 1.0, S, "zak");
    // T . B5 (:338) and T . Bn (:381) share Bn^ = T^T l2
    q.C(1.0, T4, "abkl", L2, "zabij", 0.0, BnV, "zklij");
    q.C(2.0, Vijka, "klid", BnV, "zklij", 1.0, S, "zdj");
    // the two (ov)^3 products: Pd = M12^T ld (the adjoint of utd, which enters as 2 Pd - Pd^(ab): cd, cx of the assembly),
    // Px = MDU^T Q, both held transposed
    q.C(1.0, P5(ld), "zbjai", P4(M12), "aidl", 0.0, P5(w.Pd), "zbjdl");                 // (M12^T ld_z)^T, all z: one GEMM
    q.C(2.0, P4(Td), "akbj", P5(ld), "zaibj", 0.0, XooV, "zki");
    q.C(1.0, P5(Q), "zbiaj", P4(MDU), "ajdl", 0.0, P5(w.Px), "zbidl");                  // (MDU^T Q_z)^T, all z: one GEMM
    // one-index dressings backwards
    q.C(-2.0, Vijka, "klid", XooV, "zki", 1.0, S, "zdl");
    q.C(1.0, Vijak, "kldi", XooV, "zki", 1.0, S, "zdl");
    q.C(-1.0, FOV, "kd", XooV, "zki", 1.0, S, "zdi");
    q.C(1.0, mv(Aoo, {o, v, o, v}), "kdlc", XooV, "zki", 1.0, P5(w.Px), "zdlci", "z");
    q.C(2.0, Viabc, "ladc", XvvV, "zac", 1.0, S, "zdl");
    q.C(-1.0, Viabc, "lacd", XvvV, "zac", 1.0, S, "zdl");
    q.C(-1.0, XvvV, "zac", FOV, "lc", 1.0, S, "zal");
    q.C(1.0, XvvV, "zac", slice(mv(BB, {o, v, o, v + o}), 3, 0, v), "kdlc", 1.0, P5(w.Px), "zakdl");
    // ---- the unpermuted terms (:380-383) against l2 ----------------------------------------------------------------------------------
    q.C(1.0, L2, "zabij", mv(B2, {o, o, o, o}), "klij", 1.0, D, "zabkl");
    q.C(1.0, Vijab, "kldc", BnV, "zklij", 1.0, D, "zdcij");
    // the particle ladder backwards: sum_ab V_abcd l2_abij.  With V_abcd = V_badc (every Hamiltonian the package is fed; no
    // hermiticity needed) the packed rows V+ / V- of the right build are read in the other orientation — a quarter of the flops
    // of the plain product, for dressed and transcorrelated blocks alike
    if (v_sym) e.ladder_sym_adjoint_multi(l2, k, w.Lp, w.La, dressed);
    else q.C(1.0, V("abcd"), "abcd", L2, "zabij", 1.0, D, "zcdij");
}

double EomSigma::lambda_step(const double* lam1, const double* lam2, const double* eo_host, const double* ev_host, double shift,
                             double err_scale, bool start, bool known_sym, double* out1, double* out2, double* err1, double* err2) {
    left_check();
    if (!eo_host || !ev_host || !out1 || !out2 || !err1 || !err2) throw Error("lambda_step: null argument");
    if (!start && (!lam1 || !lam2)) throw Error("lambda_step: null lambda");
    if (!start && !known_sym && !exchange_symmetric(lam2, nv, no))
        throw Error("lambda_step: lambda2 does not have the exchange symmetry l2_abij = l2_baji");
    left_prepare();
    const int64_t n = static_cast<int64_t>(no) + nv;
    std::vector<double> eps(static_cast<size_t>(n));
    for (int64_t i = 0; i < no; ++i) eps[i] = eo_host[i];
    for (int64_t a = 0; a < nv; ++a) eps[no + a] = ev_host[a];
    if (!eps_dev || eps != eps_host_) {
        if (!eps_dev) eps_dev = keep(n);
        dev::memcpy_h2d(eps_dev, eps.data(), sizeof(double) * n, e.stream);
        dev::stream_sync(e.stream);
        eps_host_ = eps;
    }
    std::optional<LeftBuild> w;
    dev::LambdaParts q;
    if (!start) {                          // (start: lambda = 0, no partial results: out = -eta / d, nothing is read)
        w.emplace(*this, 1);
        left_build(&lam1, &lam2, *w);
        q = w->parts[0];
        q.lam1 = lam1; q.lam2 = lam2;
    }
    Tmp ws(*this, dev::lambda_assemble_ws_doubles(nv)), nrm(*this, 32);
    q.cd = 2.0; q.cx = -1.0;
    q.Vijab = V("ijab").p; q.eta1 = eta1; q.eo = eps_dev; q.ev = eps_dev + no; q.shift = shift; q.err_scale = err_scale;
    q.out1 = out1; q.out2 = out2; q.err1 = err1; q.err2 = err2; q.ws = ws; q.norm_dev = nrm;
    dev::lambda_assemble(q, no, nv, e.stream);
    double r = 0.0;
    const int slot = dev::readback_start(nrm, 1, e.stream);
    dev::readback_wait(slot, &r, 1);
    return std::sqrt(r);
}

void lambda_rdm1(Engine& e, const double* t1, const double* t2, const double* lam1, const double* lam2, double ref,
                 double* gamma_host) {
    if (!t1 || !t2 || !lam1 || !lam2 || !gamma_host) throw Error("rdm1: null argument");
    const int64_t o = e.no, v = e.nv, n = o + v;
    struct Buf {
        Engine& e;
        double* p;
        Buf(Engine& e_, int64_t m) : e(e_), p(e_.scratch_get(m)) {}
        ~Buf() { e.scratch_put(p); }
    } Xvv(e, v * v), Xoo(e, o * o), Xov(e, o * v), G(e, n * n);
    const TView L1 = mv(lam1, {v, o}), L2 = mv(lam2, {v, v, o, o}), T4 = mv(t2, {v, v, o, o});
    // the lambda2 . t2 contractions: K = v o o and v v o, the engine's split-K products
    e.contract(1.0, L2, "abij", T4, "cbij", 0.0, mv(Xvv.p, {v, v}), "ac");
    e.contract(1.0, L2, "abij", T4, "abkj", 0.0, mv(Xoo.p, {o, o}), "ki");
    e.contract(2.0, L1, "ai", T4, "abij", 0.0, mv(Xov.p, {o, v}), "jb");
    e.contract(-1.0, L1, "ai", T4, "abji", 1.0, mv(Xov.p, {o, v}), "jb");
    dev::rdm1_assemble(Xvv.p, Xoo.p, Xov.p, lam1, t1, e.no, e.nv, ref, G.p, e.stream);
    dev::memcpy_d2h(gamma_host, G.p, sizeof(double) * n * n, e.stream);
    dev::stream_sync(e.stream);
}

// ==== the two-particle density (eom.h; formulas in include/pymes_amd.h, pymes_rdm2) ====================================
// G = dL/dV accumulates block by block in `raw` (one array per occupied / virtual pattern, allocated on first use), in four
// parts: the densities of the six dressed blocks, their back-transformation through t1 (walk: the adjoint of Engine::dress_V,
// index by index), the dressed-Fock part (outer products of t1 with the response density C) and the direct terms of the singles
// residual and the energy.  The [o,o,v,v] pattern is kept as [v,v,o,o] — the layout rdm2_assemble reads, which also adds that
// block's outer products and its energy term; every other stored block is (raw_pqrs + partner_qpsr) / 2 by one permute and
// one axpby.  Nothing of size v^4 exists unless the abcd block itself is asked for, nothing of size n^4 ever.
namespace {
constexpr int kOOVV = 3, kVVVV = 15;
inline int rdm2_partner(int pat) { return ((pat & 8) >> 1) | ((pat & 4) << 1) | ((pat & 2) >> 1) | ((pat & 1) << 1); }

struct Rdm2Build {
    Engine& e;
    const int64_t o, v, n;
    const double *t1, *t2, *l1, *l2;
    double* raw[16] = {nullptr};
    std::vector<double*> held;
    Rdm2Build(Engine& e_, const double* t1_, const double* t2_, const double* l1_, const double* l2_)
        : e(e_), o(e_.no), v(e_.nv), n(o + v), t1(t1_), t2(t2_), l1(l1_), l2(l2_) {}
    ~Rdm2Build() {
        for (double* p : held) e.scratch_put(p);
    }
    Rdm2Build(const Rdm2Build&) = delete;
    Rdm2Build& operator=(const Rdm2Build&) = delete;
    struct Buf {
        Engine& e;
        double* p;
        Buf(Engine& e_, int64_t m) : e(e_), p(e_.scratch_get(std::max<int64_t>(m, 1))) {}
        ~Buf() { e.scratch_put(p); }
        Buf(const Buf&) = delete;
        Buf& operator=(const Buf&) = delete;
    };
    double* get(int64_t m) {
        double* p = e.scratch_get(std::max<int64_t>(m, 1));
        held.push_back(p);
        return p;
    }
    int64_t dim(int pat, int pos) const { return ((pat >> (3 - pos)) & 1) ? v : o; }
    int64_t size(int pat) const { return dim(pat, 0) * dim(pat, 1) * dim(pat, 2) * dim(pat, 3); }
    TView view(const double* p, int pat) const { return mv(p, {dim(pat, 0), dim(pat, 1), dim(pat, 2), dim(pat, 3)}); }
    TView rawv(int pat) {
        if (!raw[pat]) {
            raw[pat] = get(size(pat));
            e.zero(mv(raw[pat], {size(pat)}));
        }
        return pat == kOOVV ? mv(raw[pat], {v, v, o, o}) : view(raw[pat], pat);
    }
    // raw[pat][sc] += al * sum A[sa] B[sb]  (sc: the block's own index order)
    void C(double al, const TView& A, const char* sa, const TView& B, const char* sb, int pat, const char* sc) {
        const char t[5] = {sc[2], sc[3], sc[0], sc[1], 0};
        e.contract(al, A, sa, B, sb, 1.0, rawv(pat), pat == kOOVV ? t : sc);
    }
    void add(int pat, const double* X) {
        if (pat == kOOVV) e.permute(1.0, view(X, pat), "pqrs", 1.0, rawv(pat), "rspq");
        else e.axpby(1.0, view(X, pat), 1.0, rawv(pat));
    }
    // X: the density of a (partly) dressed block of the pattern `pat`.  A virtual bra index sends -t1[a,k] X to the occupied source
    // index k, an occupied ket index +t1[c,i] X to the virtual source c; the positions from `start` on, each subset once.
    // no_vvvv (the walk of the abij density): the branch with both ket indices transformed is left out — it is lambda2 . t1 t1,
    // which run() sends through the abcd family together with lambda2 . t2 as lambda2 . tau, never as a v^4 array.
    void walk(int pat, const double* X, int start, bool no_vvvv = false) {
        add(pat, X);
        for (int pos = start; pos < 4; ++pos) {
            const bool virt = (pat >> (3 - pos)) & 1;
            if ((pos < 2) != virt) continue;
            if (no_vvvv && pos == 3 && ((pat >> 1) & 1)) continue;
            const int np = pat ^ (1 << (3 - pos));
            char sx[5] = "pqrs", sy[5] = "pqrs", st[3] = {0, 0, 0};
            sy[pos] = 'x';
            st[0] = pos < 2 ? sx[pos] : 'x';
            st[1] = pos < 2 ? 'x' : sx[pos];
            Buf Y(e, size(np));
            e.contract(pos < 2 ? -1.0 : 1.0, view(X, pat), sx, mv(t1, {v, o}), st, 0.0, view(Y.p, np), sy);
            walk(np, Y.p, pos + 1, no_vvvv);
        }
    }
    double *Tt = nullptr, *tau = nullptr, *Cm = nullptr, *gov = nullptr;
    void run(bool want_abcd);
    void project(int pat, double* out);
    void finish_oovv(double* out_vvoo);
};

void Rdm2Build::run(bool want_abcd) {
    const int64_t o2v2 = v * v * o * o, ov2 = o * v * o * v;
    const TView L1 = mv(l1, {v, o}), L2 = mv(l2, {v, v, o, o}), T4 = mv(t2, {v, v, o, o}), T1 = mv(t1, {v, o});
    Tt = get(o2v2);
    tau = get(o2v2);
    Cm = get(n * n);
    gov = get(o * v);
    const TView TtV = mv(Tt, {v, v, o, o}), TauV = mv(tau, {v, v, o, o}), GOV = mv(gov, {o, v});
    e.permute(2.0, T4, "abij", 0.0, TtV, "abij");
    e.permute(-1.0, T4, "baij", 1.0, TtV, "abij");
    dev::tau_build(tau, t2, t1, e.no, e.nv, e.stream);
    // ---- the one-body intermediates of lambda_rdm1 and C = the response density without the energy's 2 t1 ---------------------------
    Buf gvv(e, v * v), goo(e, o * o), Bn(e, o * o * o * o), tl(e, o * o), lt(e, v * v);
    const TView GVV = mv(gvv.p, {v, v}), GOO = mv(goo.p, {o, o}), BnV = mv(Bn.p, {o, o, o, o}), TL = mv(tl.p, {o, o}),
                LT = mv(lt.p, {v, v});
    e.contract(2.0, L2, "abij", T4, "cbij", 0.0, GVV, "ac");
    e.contract(-2.0, L2, "abij", T4, "abkj", 0.0, GOO, "ki");
    e.contract(1.0, L1, "ai", TtV, "abij", 0.0, GOV, "jb");
    e.contract(1.0, L2, "abij", T4, "abkl", 0.0, BnV, "klij");
    e.contract(1.0, T1, "ak", L1, "ai", 0.0, TL, "ki");               // (t1^T l1)[k,i]
    e.contract(1.0, L1, "ai", T1, "ci", 0.0, LT, "ac");               // (l1 t1^T)[a,c]
    const TView Cfull = mv(Cm, {n, n});
    const TView Coo = slice(slice(Cfull, 0, 0, o), 1, 0, o), Cov = slice(slice(Cfull, 0, 0, o), 1, o, n),
                Cvo = slice(slice(Cfull, 0, o, n), 1, 0, o), Cvv = slice(slice(Cfull, 0, o, n), 1, o, n);
    e.axpby(1.0, L1, 0.0, Cvo);
    e.axpby(1.0, GOO, 0.0, Coo);
    e.axpby(-1.0, TL, 1.0, Coo);
    e.axpby(1.0, GVV, 0.0, Cvv);
    e.axpby(1.0, LT, 1.0, Cvv);
    e.axpby(1.0, GOV, 0.0, Cov);
    e.contract(1.0, Coo, "ji", T1, "bi", 1.0, Cov, "jb");             // (goo - t1^T l1) t1^T
    e.contract(-1.0, T1, "aj", GVV, "ab", 1.0, Cov, "jb");            // - t1^T gvv
    // ---- 1: densities of the dressed blocks.  ijab (dressed = undressed) goes straight into its raw array -------------------------
    {
        Buf X(e, ov2);
        const TView XV = mv(X.p, {v, o, v, o});
        C(1.0, BnV, "klij", T4, "cdij", kOOVV, "klcd");
        e.contract(1.0, L2, "abij", T4, "adkj", 0.0, XV, "bidk");
        C(1.0, XV, "bidk", T4, "cbil", kOOVV, "klcd");
        e.contract(1.0, L2, "abij", TtV, "acik", 0.0, XV, "bjck");
        C(1.0, XV, "bjck", TtV, "dblj", kOOVV, "klcd");
        e.contract(1.0, L2, "abij", T4, "daki", 0.0, XV, "bjdk");
        C(2.0, XV, "bjdk", T4, "bclj", kOOVV, "klcd");
        C(-2.0, XV, "bjdk", T4, "cblj", kOOVV, "klcd");
        C(-1.0, GVV, "ad", TtV, "aclk", kOOVV, "klcd");
        C(1.0, GOO, "li", TtV, "dcik", kOOVV, "klcd");
    }
    // ---- 2: the back-transformations ----------------------------------------------------------------------------------------------
    walk(pattern_of_name("abij"), l2, 0, true);
    walk(pattern_of_name("klij"), Bn.p, 0);
    {
        Buf D(e, ov2);
        const TView P = mv(D.p, {o, v, o, v});
        e.contract(-2.0, L2, "abij", T4, "cbkj", 0.0, P, "kaic");
        e.contract(-2.0, L2, "abij", T4, "ackj", 1.0, P, "kbic");
        walk(pattern_of_name("iajb"), D.p, 0);
        e.contract(2.0, L2, "abij", TtV, "acik", 0.0, mv(D.p, {o, v, v, o}), "kbcj");
        walk(pattern_of_name("iabj"), D.p, 0);
    }
    {
        // the abcd family, Z = lambda2 . tau: Z itself only on request; its images under one and two bra transformations from
        // M1[k,b,i,j] = -sum_a t1[a,k] l2[a,b,i,j] (o v^3 o^2 and o^4 v^2 flops)
        Buf M1(e, o * v * o * o), M2(e, o * o * o * o), Y(e, o * v * v * v);
        const TView M1V = mv(M1.p, {o, v, o, o}), M2V = mv(M2.p, {o, o, o, o}), YV = mv(Y.p, {o, v, v, v});
        e.contract(-1.0, T1, "ak", L2, "abij", 0.0, M1V, "kbij");
        e.contract(-1.0, M1V, "kbij", T1, "bl", 0.0, M2V, "klij");
        e.contract(1.0, M1V, "kbij", TauV, "cdij", 0.0, YV, "kbcd");
        add(pattern_of_name("iabc"), Y.p);
        e.permute(1.0, YV, "kbcd", 1.0, rawv(pattern_of_name("aibc")), "bkdc");
        C(1.0, M2V, "klij", TauV, "cdij", kOOVV, "klcd");
        if (want_abcd) C(1.0, L2, "abij", TauV, "cdij", kVVVV, "abcd");
    }
    // ---- 3: the dressed-Fock part, V[j,p,b,q] += 2 t1[b,j] C'[p,q], V[j,p,q,b] -= t1[b,j] C[p,q] (C' = C without Xov in its ov
    // block, which the reference's f_ov dressing reads from V_iabj[j,a,b,i] instead: the last product).  The [o,o,v,v] parts are
    // rdm2_assemble's ------------------------------------------------------------------------------------------------------------------
    const TView T1x = mv(t1, {v, o, 1});
    auto outer = [&](double al, const TView& blk, int pat, const char* sc) {
        TView b3 = blk;                       // [p,q] -> [p,q,1]: the K = 1 form of an outer product
        b3.rank = 3;
        b3.dim[2] = 1;
        b3.st[2] = 1;
        C(al, T1x, "bjx", b3, "pqx", pat, sc);
    };
    outer(2.0, Coo, pattern_of_name("ijak"), "jpbq");
    outer(2.0, Cvo, pattern_of_name("iabj"), "jpbq");
    outer(2.0, Cvv, pattern_of_name("iabc"), "jpbq");
    outer(-1.0, Coo, pattern_of_name("ijka"), "jpqb");
    outer(-1.0, Cvo, pattern_of_name("iajb"), "jpqb");
    outer(-1.0, Cvv, pattern_of_name("iabc"), "jpqb");
    outer(2.0, GOV, pattern_of_name("iabj"), "jqbp");                 // 2 t1[b,j] Xov[i,a] at V_iabj[j,a,b,i]
    // ---- 4: the direct V terms of the singles residual (those of the energy: rdm2_assemble) ----------------------------------------
    C(1.0, L1, "ai", TtV, "bcij", pattern_of_name("aibc"), "ajbc");
    C(-1.0, TL, "ki", TtV, "bcij", kOOVV, "kjbc");
    C(-1.0, L1, "ai", TtV, "abjk", pattern_of_name("ijka"), "jkib");
    C(-1.0, LT, "ac", TtV, "abjk", kOOVV, "jkcb");
}

// out[a,b,i,j] = Gamma_ijab[i,j,a,b]
void Rdm2Build::finish_oovv(double* out_vvoo) {
    Buf D2(e, v * o), Cv(e, v * o);
    const TView Cfull = mv(Cm, {n, n});
    const TView Cov = slice(slice(Cfull, 0, 0, o), 1, o, n);
    e.permute(2.0, Cov, "jb", 0.0, mv(D2.p, {v, o}), "bj");
    e.permute(-2.0, mv(gov, {o, v}), "jb", 1.0, mv(D2.p, {v, o}), "bj");
    e.permute(1.0, Cov, "ja", 0.0, mv(Cv.p, {v, o}), "aj");
    dev::Rdm2Parts q;
    q.G = rawv(kOOVV).p; q.Tt = Tt; q.t1 = t1; q.D2 = D2.p; q.Cv = Cv.p; q.out = out_vvoo;
    dev::rdm2_assemble(q, e.no, e.nv, e.stream);
}

// out = (raw[pat]_pqrs + raw[partner]_qpsr) / 2 for every pattern but [o,o,v,v]
void Rdm2Build::project(int pat, double* out) {
    const TView O = view(out, pat);
    e.permute(0.5, rawv(rdm2_partner(pat)), "qpsr", 0.0, O, "pqrs");
    e.axpby(0.5, rawv(pat), 1.0, O);
}

void rdm2_check(Engine& e, const char* who, const double* t1, const double* t2, const double* lam1, const double* lam2) {
    if (!t1 || !t2 || !lam1 || !lam2) throw Error(std::string(who) + ": null argument");
    if (!dev::rdm2_assemble_ok(e.no))
        throw Error(std::string(who) + ": nocc = " + std::to_string(e.no) + " is too large for the LDS tile of rdm2_assemble (o (o + 1) + 256 "
                    "doubles in 64 KB: nocc <= " + std::to_string(PYMES_NOCC_MAX_LAMBDA) + ")");
    const int64_t d[4] = {e.nv, e.nv, e.no, e.no};
    for (const double* x : {lam2, t2}) {
        double out[2] = {0.0, 0.0};
        dev::exchange_asymmetry(x, x, d, out, e.stream);
        if (!(std::isfinite(out[1]) && out[0] <= 1e-13 * std::max(1.0, out[1])))
            throw Error(std::string(who) + (x == lam2 ? ": lambda2 does not have the exchange symmetry l2_abij = l2_baji"
                                                      : ": t2 does not have the exchange symmetry t2_abij = t2_baji"));
    }
}
}  // namespace

bool rdm2_stored(int pattern) { return pattern >= 0 && pattern < 16 && pattern <= rdm2_partner(pattern); }

void lambda_rdm2(Engine& e, const double* t1, const double* t2, const double* lam1, const double* lam2, unsigned mask,
                 double* const out[16]) {
    if (!out) throw Error("rdm2: null argument");
    if (!(mask & 0xffffu) || (mask >> 16)) throw Error("rdm2: the block mask names no block (bits 0..15: the occupied / virtual patterns)");
    for (int pat = 0; pat < 16; ++pat) {
        if (!((mask >> pat) & 1)) continue;
        if (!rdm2_stored(pat))
            throw Error("rdm2: block '" + canonical_name(pat) + "' is the image of '" + canonical_name(rdm2_partner(pat)) +
                        "' under (pq,rs) -> (qp,sr) and is not stored: ask for that one");
        if (!out[pat]) throw Error("rdm2: null output for block '" + canonical_name(pat) + "'");
        for (const double* in : {t1, t2, lam1, lam2})
            if (in == out[pat]) throw Error("rdm2: output aliases input");
        for (int q = 0; q < pat; ++q)
            if (((mask >> q) & 1) && out[q] == out[pat]) throw Error("rdm2: two outputs are the same array");
    }
    rdm2_check(e, "rdm2", t1, t2, lam1, lam2);
    const int64_t o = e.no, v = e.nv;
    Rdm2Build w(e, t1, t2, lam1, lam2);
    w.run((mask >> kVVVV) & 1);
    for (int pat = 0; pat < 16; ++pat) {
        if (!((mask >> pat) & 1)) continue;
        if (pat == kOOVV) {
            Rdm2Build::Buf S(e, v * v * o * o);
            w.finish_oovv(S.p);
            e.permute(1.0, mv(S.p, {v, v, o, o}), "abij", 0.0, mv(out[pat], {o, o, v, v}), "ijab");
        } else {
            w.project(pat, out[pat]);
        }
    }
    dev::stream_sync(e.stream);
}

double lambda_rdm2_expectation(Engine& e, const double* t1, const double* t2, const double* lam1, const double* lam2) {
    e.refuse_if_sharded("rdm2_expectation");
    e.refuse_if_direct("rdm2_expectation");
    for (int pat = 0; pat < 16; ++pat)
        if (!e.has_block(pat)) throw Error("rdm2_expectation: the operator block '" + canonical_name(pat) + "' is not set");
    rdm2_check(e, "rdm2_expectation", t1, t2, lam1, lam2);
    {
        double asym[2] = {0.0, 0.0};
        e.exchange_asymmetry_V(asym);
        if (!(std::isfinite(asym[1]) && asym[0] <= 1e-12 * std::max(1.0, asym[1])))
            throw Error("rdm2_expectation: the operator does not have the symmetry W_pqrs = W_qpsr (max |W_pqrs - W_qpsr| = " +
                        std::to_string(asym[0]) + ")");
    }
    const int64_t o = e.no, v = e.nv, npp = v * (v + 1) / 2;
    int64_t nsums = npp, largest = 1;
    for (int pat = 0; pat < kVVVV; ++pat) {
        if (!rdm2_stored(pat)) continue;
        int64_t sz = 1;
        for (int pos = 0; pos < 4; ++pos) sz *= ((pat >> (3 - pos)) & 1) ? v : o;
        nsums += dev::rdm2_contract_sums(sz);
        largest = std::max(largest, sz);
    }
    Rdm2Build w(e, t1, t2, lam1, lam2);
    w.run(false);
    Rdm2Build::Buf ws(e, nsums + 1), G(e, largest);
    int64_t at = 0;
    for (int pat = 0; pat < kVVVV; ++pat) {
        if (!rdm2_stored(pat)) continue;
        const double wgt = rdm2_partner(pat) == pat ? 1.0 : 2.0;      // (a block and its image contribute the same sum)
        const int64_t sz = w.size(pat);
        if (pat == kOOVV) {
            Rdm2Build::Buf S(e, sz);
            w.finish_oovv(S.p);
            e.permute(1.0, mv(S.p, {v, v, o, o}), "abij", 0.0, mv(G.p, {o, o, v, v}), "ijab");
        } else {
            w.project(pat, G.p);
        }
        dev::rdm2_contract(G.p, e.block(pat).p, sz, wgt, ws.p + at, e.stream);
        at += dev::rdm2_contract_sums(sz);
    }
    {
        // the abcd block never exists: sum Gamma_abcd W_abcd = sum_abij l2_abij (sum_cd W_abcd tau_cdij), the inner sum through the
        // pair-packed ladder on W's V+ / V- packs (a quarter of the flops of the plain product), the outer one on the packed rows
        Rdm2Build::Buf L(e, npp * o * o);
        e.ladder_sym(w.tau, L.p, 0, npp, false);
        dev::rdm2_contract_packed(lam2, L.p, e.no, e.nv, ws.p + at, e.stream);
        at += npp;
    }
    dev::rdm2_contract_finish(ws.p, at, ws.p + nsums, e.stream);
    double r = 0.0;
    const int slot = dev::readback_start(ws.p + nsums, 1, e.stream);
    dev::readback_wait(slot, &r, 1);
    return r;
}

// ---- transition densities of k roots (eom.h): the v o o / v v o-contracted intermediates as engine products with the
// k vectors stacked (one GEMM per product), then one assembly launch for both densities of all roots ---------------------------
void transition_densities(Engine& e, const double* t1, const double* t2, const double* lam1, const double* lam2, int k,
                          const double* const* l1, const double* const* l2, const double* const* r1, const double* const* r2,
                          double* gl_host, double* gr_host, double* r0_host) {
    if (!t1 || !t2 || !lam1 || !lam2 || !l1 || !l2 || !r1 || !r2 || !gl_host || !gr_host || !r0_host)
        throw Error("tdm1: null argument");
    if (k < 1 || k > 64) throw Error("tdm1: 1 <= k <= 64 roots per call");
    for (int z = 0; z < k; ++z)
        if (!l1[z] || !l2[z] || !r1[z] || !r2[z]) throw Error("tdm1: null vector");
    const int64_t o = e.no, v = e.nv, n = o + v, K = k, n1 = v * o, n2 = v * v * o * o;
    struct Buf {
        Engine& e;
        double* p;
        Buf(Engine& e_, int64_t m) : e(e_), p(e_.scratch_get(m)) {}
        ~Buf() { e.scratch_put(p); }
    } L1(e, K * n1), R1(e, K * n1), L2(e, K * n2), R2(e, K * n2), Xvv(e, K * v * v), Xoo(e, K * o * o), Xov(e, K * n1),
        Yvv(e, v * v), Yoo(e, o * o), Yov(e, n1), Zvv(e, K * v * v), Zoo(e, K * o * o), Zov(e, K * n1), Le(e, K * n1),
        Eov(e, K * n1), G(e, 2 * K * n * n + K);
    for (int z = 0; z < k; ++z) {
        dev::memcpy_d2d(L1.p + z * n1, l1[z], sizeof(double) * n1, e.stream);
        dev::memcpy_d2d(R1.p + z * n1, r1[z], sizeof(double) * n1, e.stream);
        dev::memcpy_d2d(L2.p + z * n2, l2[z], sizeof(double) * n2, e.stream);
        dev::memcpy_d2d(R2.p + z * n2, r2[z], sizeof(double) * n2, e.stream);
    }
    const TView T4 = mv(t2, {v, v, o, o}), LAM1 = mv(lam1, {v, o}), LAM2 = mv(lam2, {v, v, o, o});
    const TView L1v = mv(L1.p, {K, v, o}), R1v = mv(R1.p, {K, v, o}), L2v = mv(L2.p, {K, v, v, o, o}), R2v = mv(R2.p, {K, v, v, o, o});
    auto vv = [&](double* p) { return mv(p, {K, v, v}); };
    auto oo = [&](double* p) { return mv(p, {K, o, o}); };
    auto ov = [&](double* p) { return mv(p, {K, o, v}); };
    // l_z . t
    e.contract(1.0, L2v, "zabij", T4, "cbij", 0.0, vv(Xvv.p), "zac");
    e.contract(1.0, L2v, "zabij", T4, "abkj", 0.0, oo(Xoo.p), "zki");
    e.contract(2.0, L1v, "zai", T4, "abij", 0.0, ov(Xov.p), "zjb");
    e.contract(-1.0, L1v, "zai", T4, "abji", 1.0, ov(Xov.p), "zjb");
    // lambda . t
    e.contract(1.0, LAM2, "abij", T4, "cbij", 0.0, mv(Yvv.p, {v, v}), "ac");
    e.contract(1.0, LAM2, "abij", T4, "abkj", 0.0, mv(Yoo.p, {o, o}), "ki");
    e.contract(2.0, LAM1, "ai", T4, "abij", 0.0, mv(Yov.p, {o, v}), "jb");
    e.contract(-1.0, LAM1, "ai", T4, "abji", 1.0, mv(Yov.p, {o, v}), "jb");
    // lambda . r_z
    e.contract(1.0, LAM2, "abij", R2v, "zcbij", 0.0, vv(Zvv.p), "zac");
    e.contract(1.0, LAM2, "abij", R2v, "zabkj", 0.0, oo(Zoo.p), "zki");
    e.contract(2.0, LAM1, "ai", R2v, "zabij", 0.0, ov(Zov.p), "zjb");
    e.contract(-1.0, LAM1, "ai", R2v, "zabji", 1.0, ov(Zov.p), "zjb");
    e.contract(2.0, LAM2, "abij", R1v, "zai", 0.0, mv(Le.p, {K, v, o}), "zbj");
    e.contract(2.0, mv(Le.p, {K, v, o}), "zai", T4, "abij", 0.0, ov(Eov.p), "zjb");
    e.contract(-1.0, mv(Le.p, {K, v, o}), "zai", T4, "abji", 1.0, ov(Eov.p), "zjb");
    dev::Tdm1Parts q;
    q.t1 = t1; q.lam1 = lam1; q.L1 = L1.p; q.R1 = R1.p;
    q.Xvv = Xvv.p; q.Xoo = Xoo.p; q.Xov = Xov.p; q.Yvv = Yvv.p; q.Yoo = Yoo.p; q.Yov = Yov.p;
    q.Zvv = Zvv.p; q.Zoo = Zoo.p; q.Zov = Zov.p; q.Le = Le.p; q.Eov = Eov.p;
    q.gl = G.p; q.gr = G.p + K * n * n; q.r0 = G.p + 2 * K * n * n;
    dev::tdm1_assemble(q, k, e.no, e.nv, e.stream);
    dev::memcpy_d2h(gl_host, q.gl, sizeof(double) * K * n * n, e.stream);
    dev::memcpy_d2h(gr_host, q.gr, sizeof(double) * K * n * n, e.stream);
    dev::memcpy_d2h(r0_host, q.r0, sizeof(double) * K, e.stream);
    dev::stream_sync(e.stream);
}

// ---- the property vectors of the linear response function (eom.h): the T1 dressing of the k operators on the host
// (k n^2 numbers), the o v-contracted intermediates as engine products with the operators stacked, one launch for the singles and
// g0, one launch each for xi2 (T = t2) and eta2 (T = lambda2) -----------------------------------------------------------------------
void response_vectors(Engine& e, const double* t1, const double* t2, const double* lam1, const double* lam2, int k,
                      const double* ops_host, double* const* xi1, double* const* xi2, double* const* eta1, double* const* eta2,
                      double* g0_host) {
    if (!t1 || !t2 || !lam1 || !lam2 || !ops_host || !xi1 || !xi2 || !eta1 || !eta2 || !g0_host)
        throw Error("response_vectors: null argument");
    if (k < 1 || k > dev::kResponseOps) throw Error("response_vectors: 1 <= k <= 64 operators per call");
    std::vector<const double*> outs;
    for (int z = 0; z < k; ++z) {
        if (!xi1[z] || !xi2[z] || !eta1[z] || !eta2[z]) throw Error("response_vectors: null vector");
        for (const double* out : {xi1[z], xi2[z], eta1[z], eta2[z]}) {
            for (const double* in : {t1, t2, lam1, lam2})
                if (in == out) throw Error("response_vectors: output aliases input");
            for (const double* other : outs)
                if (other == out) throw Error("response_vectors: two outputs are the same array");
            outs.push_back(out);
        }
    }
    const int64_t o = e.no, v = e.nv, n = o + v, K = k, n1 = v * o;
    {
        const int64_t d[4] = {v, v, o, o};
        for (const double* x : {lam2, t2}) {
            double out[2] = {0.0, 0.0};
            dev::exchange_asymmetry(x, x, d, out, e.stream);
            if (!(std::isfinite(out[1]) && out[0] <= 1e-13 * std::max(1.0, out[1])))
                throw Error(x == lam2 ? "response_vectors: lambda2 does not have the exchange symmetry l2_abij = l2_baji"
                                      : "response_vectors: t2 does not have the exchange symmetry t2_abij = t2_baji");
        }
    }
    // the dressed blocks: O~_ov = O_ov, O~_oo = O_oo + O_ov t1, O~_vv = O_vv - t1 O_ov, O~_vo = O_vo + O_vv t1 - t1 O~_oo
    std::vector<double> th(static_cast<size_t>(n1));
    dev::memcpy_d2h(th.data(), t1, sizeof(double) * n1, e.stream);
    dev::stream_sync(e.stream);
    const size_t soo = static_cast<size_t>(K * o * o), svv = static_cast<size_t>(K * v * v), svo = static_cast<size_t>(K * n1);
    std::vector<double> hoo(soo), hooT(soo), hvv(svv), hvvT(svv), hov(svo), hvo(svo);
    for (int64_t z = 0; z < K; ++z) {
        const double* O = ops_host + z * n * n;
        double *oo = hoo.data() + z * o * o, *ooT = hooT.data() + z * o * o, *vv = hvv.data() + z * v * v,
               *vvT = hvvT.data() + z * v * v, *ov = hov.data() + z * n1, *vo = hvo.data() + z * n1;
        for (int64_t j = 0; j < o; ++j) {
            for (int64_t b = 0; b < v; ++b) ov[j * v + b] = O[j * n + o + b];
            for (int64_t i = 0; i < o; ++i) {
                double s = O[j * n + i];
                for (int64_t b = 0; b < v; ++b) s += ov[j * v + b] * th[b * o + i];
                oo[j * o + i] = s;
                ooT[i * o + j] = s;
            }
        }
        for (int64_t a = 0; a < v; ++a) {
            for (int64_t b = 0; b < v; ++b) {
                double s = O[(o + a) * n + o + b];
                for (int64_t j = 0; j < o; ++j) s -= th[a * o + j] * ov[j * v + b];
                vv[a * v + b] = s;
                vvT[b * v + a] = s;
            }
            for (int64_t i = 0; i < o; ++i) {
                double s = O[(o + a) * n + i];
                for (int64_t b = 0; b < v; ++b) s += O[(o + a) * n + o + b] * th[b * o + i];
                for (int64_t j = 0; j < o; ++j) s -= th[a * o + j] * oo[j * o + i];
                vo[a * o + i] = s;
            }
        }
    }
    struct Buf {
        Engine& e;
        double* p;
        Buf(Engine& e_, int64_t m) : e(e_), p(e_.scratch_get(m)) {}
        ~Buf() { e.scratch_put(p); }
    } Ooo(e, K * o * o), OooT(e, K * o * o), Ovv(e, K * v * v), OvvT(e, K * v * v), Oov(e, K * n1), Ovo(e, K * n1), XI1(e, K * n1),
        L2X(e, K * n1), Yvv(e, v * v), Yoo(e, o * o), Yov(e, n1), G(e, 2 * K);
    auto up = [&](double* d, const std::vector<double>& h) { dev::memcpy_h2d(d, h.data(), sizeof(double) * h.size(), e.stream); };
    up(Ooo.p, hoo); up(OooT.p, hooT); up(Ovv.p, hvv); up(OvvT.p, hvvT); up(Oov.p, hov); up(Ovo.p, hvo); up(XI1.p, hvo);
    dev::stream_sync(e.stream);                 // (the host blocks die with this scope's vectors only after the copies have read them)
    const TView T4 = mv(t2, {v, v, o, o}), LAM1 = mv(lam1, {v, o}), LAM2 = mv(lam2, {v, v, o, o});
    const TView W = mv(Oov.p, {K, o, v}), X1 = mv(XI1.p, {K, v, o});
    // xi1_z = O~_vo + (2 t - t^(ij)) . O~_ov
    e.contract(2.0, T4, "abij", W, "zjb", 1.0, X1, "zai");
    e.contract(-1.0, T4, "abji", W, "zjb", 1.0, X1, "zai");
    // Y = X(lambda1, lambda2) of transition_densities
    e.contract(1.0, LAM2, "abij", T4, "cbij", 0.0, mv(Yvv.p, {v, v}), "ac");
    e.contract(1.0, LAM2, "abij", T4, "abkj", 0.0, mv(Yoo.p, {o, o}), "ki");
    e.contract(2.0, LAM1, "ai", T4, "abij", 0.0, mv(Yov.p, {o, v}), "jb");
    e.contract(-1.0, LAM1, "ai", T4, "abji", 1.0, mv(Yov.p, {o, v}), "jb");
    // lambda2 . xi1_z
    e.contract(1.0, LAM2, "caki", X1, "zai", 0.0, mv(L2X.p, {K, v, o}), "zck");
    dev::ResponseSingles q;
    q.Ooo = Ooo.p; q.Oov = Oov.p; q.Ovo = Ovo.p; q.Ovv = Ovv.p; q.lam1 = lam1; q.Yoo = Yoo.p; q.Yvv = Yvv.p; q.Yov = Yov.p;
    q.XI1 = XI1.p; q.L2X = L2X.p; q.g0 = G.p; q.mg0 = G.p + K;
    dev::response_singles(q, k, e.no, e.nv, xi1, eta1, e.stream);
    dev::response_doubles(t2, Ovv.p, Ooo.p, nullptr, nullptr, nullptr, k, e.no, e.nv, xi2, e.stream);
    dev::response_doubles(lam2, OvvT.p, OooT.p, lam1, Oov.p, G.p + K, k, e.no, e.nv, eta2, e.stream);
    const int slot = dev::readback_start(G.p, k, e.stream);
    dev::readback_wait(slot, g0_host, k);       // (enqueued behind the launches: the scratch buffers are free to go back)
}

// ---- the dots and the fused update of a response sweep (eom.h): the systems' descriptions go to the device in one copy -----------
namespace {
struct ResponseLaunch {
    Engine& e;
    double *sys, *ws, *out;
    ResponseLaunch(Engine& e_, int n, const dev::ResponseSystem* host, int64_t len, int64_t nout)
        : e(e_),
          sys(e_.scratch_get((static_cast<int64_t>(sizeof(dev::ResponseSystem)) * n + 7) / 8)),
          ws(e_.scratch_get(std::max<int64_t>(dev::response_ws_doubles(n, len), 1))),
          out(e_.scratch_get(nout)) {
        dev::memcpy_h2d(sys, host, sizeof(dev::ResponseSystem) * n, e.stream);
    }
    ~ResponseLaunch() {
        e.scratch_put(out);
        e.scratch_put(ws);
        e.scratch_put(sys);
    }
    const dev::ResponseSystem* systems() const { return reinterpret_cast<const dev::ResponseSystem*>(sys); }
};
// the results of a sweep: through the pinned read-back ring where they fit a slot (128 doubles), else one copy; ONE synchronisation
void response_read(Engine& e, const double* src, double* host, int64_t count) {
    if (count <= 128) {
        const int slot = dev::readback_start(src, static_cast<int>(count), e.stream);
        dev::readback_wait(slot, host, static_cast<int>(count));
        return;
    }
    dev::memcpy_d2h(host, src, sizeof(double) * count, e.stream);
    dev::stream_sync(e.stream);
}
void response_check(const char* who, int n, const dev::ResponseSystem* sys, bool update) {
    if (!sys) throw Error(std::string(who) + ": null argument");
    if (n < 1 || n > 4096) throw Error(std::string(who) + ": 1 <= n <= 4096 systems per call");
    for (int s = 0; s < n; ++s) {
        const dev::ResponseSystem& S = sys[s];
        const bool cplx = S.r[1] != nullptr, step = S.p[0] != nullptr;
        if (S.nh < 0 || S.nh > dev::kResponseHist) throw Error(std::string(who) + ": 0 <= nh <= " + std::to_string(dev::kResponseHist) + " stored directions");
        if (!S.r[0] || (update && (!S.x[0] || !S.pn[0])) || (!update && !step) || (step && !S.ap[0]))
            throw Error(std::string(who) + ": null vector");
        if (cplx ? ((update && (!S.x[1] || !S.pn[1])) || (step && (!S.p[1] || !S.ap[1])))
                 : (S.x[1] || S.p[1] || S.ap[1] || S.pn[1] || S.z[1] != 0.0 || S.alpha[1] != 0.0))
            throw Error(std::string(who) + ": a system is real (every imaginary part null, Im z = 0) or complex (none null)");
        for (int j = 0; j < (step ? S.nh : 0); ++j) {
            if (!S.hp[j][0] || !S.hq[j][0] || cplx != (S.hp[j][1] != nullptr) || cplx != (S.hq[j][1] != nullptr))
                throw Error(std::string(who) + ": null stored direction");
            if (!cplx && S.g[j][1] != 0.0) throw Error(std::string(who) + ": a real system with a complex coefficient");
        }
    }
}
}  // namespace

void response_dots(Engine& e, int n, const dev::ResponseSystem* sys, int64_t n1, int64_t off2, int64_t len, double* dots_host) {
    if (!dots_host) throw Error("response_dots: null argument");
    response_check("response_dots", n, sys, false);
    ResponseLaunch w(e, n, sys, len, static_cast<int64_t>(n) * dev::kResponseDots);
    dev::memset_zero(w.out, sizeof(double) * n * dev::kResponseDots, e.stream);        // (a row is written up to 2 (nh + 2) only)
    dev::response_dots(w.systems(), n, n1, off2, len, w.ws, w.out, e.stream);
    response_read(e, w.out, dots_host, static_cast<int64_t>(n) * dev::kResponseDots);
}

void response_update(Engine& e, int n, const dev::ResponseSystem* sys, const double* d, double floor, int64_t n1, int64_t off2,
                     int64_t len, double* norms_host) {
    if (!d || !norms_host) throw Error("response_update: null argument");
    response_check("response_update", n, sys, true);
    ResponseLaunch w(e, n, sys, len, n);
    dev::response_update(w.systems(), n, d, floor, n1, off2, len, w.ws, w.out, e.stream);
    response_read(e, w.out, norms_host, n);
}

// ---- the Davidson correction of n roots over flat vectors (eom.h), sixteen roots per launch ----------------------------------------
void davidson_correction(Engine& e, int n, const double* const* s, const double* const* r, const double* w_host, const double* d,
                         double shift, double* const* q, int64_t n1, int64_t off2, int64_t len, double* norms_host) {
    for (int lo = 0; lo < n; lo += 16) {
        const int g = std::min(16, n - lo);
        struct Buf {
            Engine& e;
            double* p;
            Buf(Engine& e_, int64_t m) : e(e_), p(e_.scratch_get(std::max<int64_t>(m, 1))) {}
            ~Buf() { e.scratch_put(p); }
        } ws(e, dev::ipea_correction_ws_doubles(g, len)), out(e, 32);
        dev::ipea_correction(g, s + lo, r + lo, w_host + lo, d, shift, q + lo, n1, off2, len, ws.p, out.p, e.stream);
        const int slot = dev::readback_start(out.p, 2 * g, e.stream);
        dev::readback_wait(slot, norms_host + 2 * lo, 2 * g);
    }
}

// ---- eom_ccsd.py:169-198 (singles) and :200-266 (doubles) on the device ---------------------------------------------------------
void eom_diagonals(Engine& e, const double* f_host, const double* t2, bool dressed, double* d1, double* d2) {
    if (!f_host || !t2 || !d1 || !d2) throw Error("eom diagonals: null argument");
    const int64_t o = e.no, v = e.nv, n = o + v;
    std::vector<double> h(static_cast<size_t>(v * o));
    for (int64_t a = 0; a < v; ++a)
        for (int64_t i = 0; i < o; ++i) h[a * o + i] = f_host[(o + a) * n + o + a] - f_host[i * n + i];
    ArenaScope scope(e.arena);
    double *dai = e.arena.alloc(v * o), *iaai = e.arena.alloc(v * o), *iaia = e.arena.alloc(v * o), *ijij = e.arena.alloc(o * o),
           *abab = e.arena.alloc(v * v), *ws = e.arena.alloc(dev::eom_diag_ws_doubles(e.no, e.nv));
    dev::memcpy_h2d(dai, h.data(), sizeof(double) * v * o, e.stream);
    dev::stream_sync(e.stream);
    // the four diagonal slices of other blocks, gathered through strided views (o v / o^2 / v^2 numbers)
    auto gather = [&](const char* name, int64_t d0, int64_t d1_, int64_t s0, int64_t s1_, double* out) {
        const TView blk = e.block(pattern_of_name(name), dressed);
        const int64_t dims[2] = {d0, d1_}, st[2] = {s0, s1_};
        e.permute(1.0, make_view(blk.p, 2, dims, st), "xy", 0.0, mv(out, {d0, d1_}), "xy");
    };
    gather("iabj", v, o, v * o + o, v * v * o + 1, iaai);          // [a,i] <- V[i,a,a,i]
    gather("iajb", v, o, o * v + 1, v * o * v + v, iaia);          // [a,i] <- V[i,a,i,a]
    gather("klij", o, o, o * o * o + o, o * o + 1, ijij);          // [i,j] <- V[i,j,i,j]
    gather("abcd", v, v, v * v * v + v, v * v + 1, abab);          // [a,b] <- V[a,b,a,b]
    dev::eom_diagonals(e.block(pattern_of_name("ijab"), dressed).p, t2, dai, iaai, iaia, ijij, abab, d1, d2, e.no, e.nv, ws,
                       e.stream);
}

// ==== IP- / EA-EOM-CCSD (eom.h, IpEaSigma) =============================================================================
// The 7 + 32 terms per operator that the EE sigma above leaves in the sector with one non-interacting orbital (tables in
// include/pymes_amd.h), factorised.  With R[z,x,y,w] = r2_z[x,y,w], Rx its (x,y) transpose and Rt = 2 R - Rx every term lands
// either in D[z,x,y,w] or in the transposed partial E[z,y,x,w]; the assembly kernel adds the two (and the abcd product of EA).
double* IpEaSigma::keep(int64_t doubles) {
    double* p = e.scratch_get(doubles);
    owned_.push_back(p);
    return p;
}
struct IpEaSigma::Tmp {
    Engine& e;
    double* p;
    Tmp(IpEaSigma& s, int64_t n) : e(s.e), p(s.e.scratch_get(std::max<int64_t>(n, 1))) {}
    ~Tmp() { e.scratch_put(p); }
    Tmp(const Tmp&) = delete;
    Tmp& operator=(const Tmp&) = delete;
    operator double*() const { return p; }
};

TView IpEaSigma::V(const char* name) const { return e.block(pattern_of_name(name), dressed); }

const std::vector<const char*>& IpEaSigma::blocks(Kind kind) {
    static const std::vector<const char*> ip{"ijab", "iabj", "iajb", "ijka", "ijak", "iabc", "iajk", "klij"};
    static const std::vector<const char*> ea{"ijab", "iabj", "iajb", "ijka", "iabc", "abic", "abcd"};
    return kind == IP ? ip : ea;
}

IpEaSigma::~IpEaSigma() {
    for (double* p : owned_) e.scratch_put(p);
}

IpEaSigma::IpEaSigma(Engine& eng, Kind kind_, const double* f_host, const double* t2, bool dressed_)
    : e(eng), kind(kind_), no(eng.no), nv(eng.nv), dressed(dressed_), T(t2) {
    if (!f_host || !t2) throw Error("ip/ea sigma: null Fock matrix / amplitudes");
    const char* who = kind == IP ? "IP-EOM-CCSD sigma" : "EA-EOM-CCSD sigma";
    if (kind == EA) e.refuse_if_sharded(who);
    if (kind == EA) e.refuse_if_direct(who);
    for (const char* name : blocks(kind))
        if (!e.has_block(pattern_of_name(name), dressed))
            throw Error(std::string(who) + ": the " + (dressed ? "dressed " : "") + "block '" + name + "' is missing");
    // the symmetries the restricted operator needs (without them it is not even exchange-symmetric): once per prepare
    auto asym = [&](const double* A, const double* B, int64_t d0, int64_t d1, int64_t d2, int64_t d3) {
        const int64_t d[4] = {d0, d1, d2, d3};
        double out[2] = {0.0, 0.0};
        dev::exchange_asymmetry(A, B, d, out, e.stream);
        return std::isfinite(out[1]) && out[0] <= 1e-12 * std::max(1.0, out[1]);
    };
    const int64_t o = no, v = nv;
    bool v_ok = asym(V("ijab").p, V("ijab").p, o, o, v, v);
    if (kind == IP) v_ok = v_ok && asym(V("klij").p, V("klij").p, o, o, o, o) && asym(V("ijka").p, V("ijak").p, o, o, o, v);
    else v_ok = v_ok && asym(V("abcd").p, V("abcd").p, v, v, v, v);
    if (!v_ok) throw Error(std::string(who) + ": the integrals lack the exchange symmetry V_pqrs = V_qpsr");
    if (!asym(T, T, v, v, o, o)) throw Error(std::string(who) + ": the amplitudes lack the exchange symmetry T_abij = T_baji");
    try {
        hoist(f_host);
    } catch (...) {
        for (double* p : owned_) e.scratch_put(p);
        owned_.clear();
        throw;
    }
}

void IpEaSigma::hoist(const double* f_host) {
    const int64_t o = no, v = nv, n = o + v, ov = o * v, ov2 = ov * ov;
    const Ops q{e};
    std::vector<double> h(static_cast<size_t>(std::max(v * v, std::max(o * v, o * o))));
    auto upload = [&](int64_t r0, int64_t nr, int64_t c0, int64_t nc, bool transposed = false) {
        for (int64_t r = 0; r < nr; ++r)
            for (int64_t c = 0; c < nc; ++c) h[transposed ? c * nr + r : r * nc + c] = f_host[(r0 + r) * n + c0 + c];
        double* d = keep(nr * nc);
        dev::memcpy_h2d(d, h.data(), sizeof(double) * nr * nc, e.stream);
        dev::stream_sync(e.stream);            // (h is reused)
        return d;
    };
    const TView Vijab = V("ijab"), Viabj = V("iabj"), Viajb = V("iajb"), Vijka = V("ijka");
    const TView T4 = mv(T, {v, v, o, o});
    // L_oo[l,i] = f_oo + (2 V_klcd - V_kldc) t_cdki,   L_vv[a,d] = f_vv - (2 V_klcd t_cakl - V_klcd t_ackl)
    Loo = upload(0, o, 0, o);
    Lvv = upload(o, v, o, v);
    fov = upload(0, o, o, v);
    fovT = upload(0, o, o, v, true);
    q.C(2.0, Vijab, "klcd", T4, "cdki", 1.0, mv(Loo, {o, o}), "li");
    q.C(-1.0, Vijab, "kldc", T4, "cdki", 1.0, mv(Loo, {o, o}), "li");
    q.C(-2.0, Vijab, "klcd", T4, "cakl", 1.0, mv(Lvv, {v, v}), "ad");
    q.C(1.0, Vijab, "klcd", T4, "ackl", 1.0, mv(Lvv, {v, v}), "ad");
    // the (ov) x (ov) pair matrices of EomSigma (M1, M_C, M_D, U there), combined for the three products of one build:
    //   PA = 2 M1 + M2 = 2 M1 + M_D - 2 M_C - U,   PB = M_C - M1,   MDU = M_D - U        as [(a,i),(d,l)]
    PA = keep(ov2);
    PB = keep(ov2);
    MDU = keep(ov2);
    auto P4 = [&](double* p) { return mv(p, {v, o, v, o}); };
    {
        Tmp M1(*this, ov2), MC(*this, ov2), MD(*this, ov2), Ud(*this, ov2);
        {
            Tmp Vd(*this, ov2), Vx(*this, ov2), Tdl(*this, ov2), Txl(*this, ov2), TAB(*this, ov2);
            q.P(1.0, T4, "abij", 0.0, P4(Tdl), "aibj");
            q.P(1.0, T4, "abij", 0.0, P4(Txl), "ajbi");
            q.P(1.0, Vijab, "klcd", 0.0, P4(Vd), "ckdl");
            q.P(1.0, Vijab, "klcd", 0.0, P4(Vx), "cldk");
            q.P(2.0, P4(Tdl), "ckai", 0.0, P4(TAB), "aick");                     // 2 T[c,a,k,i] - T[a,c,k,i] as [(a,i),(c,k)]
            q.P(-1.0, P4(Txl), "aick", 1.0, P4(TAB), "aick");
            q.P(1.0, Viabj, "kaci", 0.0, P4(M1), "aick");
            q.C(1.0, P4(TAB), "aick", P4(Vd), "ckdl", 1.0, P4(M1), "aidl");
            q.C(1.0, P4(Tdl), "ckai", P4(Vx), "dlck", 0.0, P4(MC), "aidl");
            q.C(1.0, P4(Txl), "aick", P4(Vx), "dlck", 0.0, P4(MD), "aidl");
            q.P(1.0, Viajb, "kaic", 0.0, P4(Ud), "aick");
        }
        if (kind == EA) {
            q.L(PA, {M1.p, MD.p, MC.p, Ud.p}, {2.0, 1.0, -2.0, -1.0}, ov2);
            q.L(PB, {MC.p, M1.p}, {1.0, -1.0}, ov2);
            q.L(MDU, {MD.p, Ud.p}, {1.0, -1.0}, ov2);
        } else {                     // IP: pair index (i,a), the order of r2[.,i,a]
            Tmp X(*this, ov2);
            auto P4o = [&](double* p) { return mv(p, {o, v, o, v}); };
            q.L(X, {M1.p, MD.p, MC.p, Ud.p}, {2.0, 1.0, -2.0, -1.0}, ov2);
            q.P(1.0, P4(X), "aidl", 0.0, P4o(PA), "iald");
            q.L(X, {MC.p, M1.p}, {1.0, -1.0}, ov2);
            q.P(1.0, P4(X), "aidl", 0.0, P4o(PB), "iald");
            q.L(X, {MD.p, Ud.p}, {1.0, -1.0}, ov2);
            q.P(1.0, P4(X), "aidl", 0.0, P4o(MDU), "iald");
        }
    }
    if (kind == IP) {
        const TView Vijak = V("ijak"), Viajk = V("iajk"), Vklij = V("klij");
        B2 = keep(o * o * o * o);                                               // W_klij = V_klij + V_klcd t_cdij
        q.P(1.0, Vklij, "klij", 0.0, mv(B2, {o, o, o, o}), "klij");
        q.C(1.0, Vijab, "klcd", T4, "cdij", 1.0, mv(B2, {o, o, o, o}), "klij");
        // TA[(c | l),i,j,b]: rows c: t[c,b,i,j] (for Y_c, below); rows l: everything r1_l multiplies except the V_lacd.t term,
        //   A[l,i,j,b] = (-2 V_klci t_cbkj + V_klic t_cbkj + V_kldi t_bdkj) + V_klid t_adkj|(j,b,i) - V_iajk[l,b,i,j] - f_lc t_cbij
        TA = keep((v + o) * o * o * v);
        const TView TAv = mv(TA, {v + o, o, o, v});
        const TView At = slice(TAv, 0, 0, v), Al = slice(TAv, 0, v, v + o);
        q.P(1.0, T4, "cbij", 0.0, At, "cijb");
        Tmp A3(*this, o * o * v * o), A4(*this, o * o * v * o);
        q.C(-2.0, Vijak, "klci", T4, "cbkj", 0.0, mv(A3, {o, o, v, o}), "libj");
        q.C(1.0, Vijka, "klic", T4, "cbkj", 1.0, mv(A3, {o, o, v, o}), "libj");
        q.C(1.0, Vijak, "kldi", T4, "bdkj", 1.0, mv(A3, {o, o, v, o}), "libj");
        q.C(1.0, Vijka, "klid", T4, "adkj", 0.0, mv(A4, {o, o, v, o}), "liaj");
        q.P(1.0, mv(A3, {o, o, v, o}), "libj", 0.0, Al, "lijb");
        q.P(1.0, mv(A4, {o, o, v, o}), "ljbi", 1.0, Al, "lijb");
        q.P(-1.0, Viajk, "lbij", 1.0, Al, "lijb");
        q.C(-1.0, mv(fov, {o, v}), "lc", T4, "cbij", 1.0, Al, "lijb");
        // BB[(l,k,d),(c | i)] = [-V_lkcd | -V_ijka[l,k,i,d]]: Y_c and the singles term from ONE pass over Rt
        BB = keep(o * o * v * (v + o));
        const TView BBv = mv(BB, {o, o, v, v + o});
        q.P(-1.0, Vijab, "lkcd", 0.0, slice(BBv, 3, 0, v), "lkdc");
        q.P(-1.0, Vijka, "lkid", 0.0, slice(BBv, 3, v, v + o), "lkdi");
    } else {
        // pair layouts of T on [(c,k),(b,j)]: Td = t[c,b,k,j], Tx = t[b,c,k,j], TT = 2 Td - Tx
        Td = keep(ov2);
        Tx = keep(ov2);
        TT = keep(ov2);
        q.P(1.0, T4, "cbkj", 0.0, P4(Td), "ckbj");
        q.P(1.0, T4, "bckj", 0.0, P4(Tx), "ckbj");
        q.L(TT, {Td, Tx}, {2.0, -1.0}, ov2);
    }
}

int IpEaSigma::stack_limit() const {
    const double free_b = static_cast<double>(dev::mem_free_bytes()) + static_cast<double>(e.scratch_free_bytes());
    const double per_vector = 8.0 * (12.0 * static_cast<double>(n2()) + static_cast<double>(nv) * nv * nv);
    return static_cast<int>(std::max(1.0, std::min(16.0, std::floor(free_b / 2.0 / std::max(per_vector, 1.0)))));
}

void IpEaSigma::apply(int k, const double* const* r1, const double* const* r2, double* const* s1, double* const* s2) {
    if (k < 1) return;
    for (int z = 0; z < k; ++z)
        if (!r1[z] || !r2[z] || !s1[z] || !s2[z]) throw Error("ip/ea sigma: null vector");
    const int step = stack_limit();
    for (int lo = 0; lo < k; lo += step) {
        const int g = std::min(k - lo, step);
        if (kind == IP) apply_ip(g, r1 + lo, r2 + lo, s1 + lo, s2 + lo);
        else apply_ea(g, r1 + lo, r2 + lo, s1 + lo, s2 + lo);
    }
}

void IpEaSigma::apply_ip(int k, const double* const* r1, const double* const* r2, double* const* s1, double* const* s2) {
    const int64_t o = no, v = nv, K = k, n2 = o * o * v;
    const Ops q{e};
    Tmp U1(*this, K * o), R(*this, K * n2), Rx(*this, K * n2), Rt(*this, K * n2), D(*this, K * n2), E(*this, K * n2),
        S1(*this, K * o), YS(*this, K * (v + o)), XU(*this, K * (v + o)), Z(*this, K * v * v * v);
    dev::ipea_pack(k, r1, r2, no, nv, no, U1, R, Rx, Rt, nullptr, e.stream);
    const TView U1v = mv(U1, {K, o}), Rv = mv(R, {K, o, o, v}), Rxv = mv(Rx, {K, o, o, v}), Rtv = mv(Rt, {K, o, o, v}),
                Dv = mv(D, {K, o, o, v}), Ev = mv(E, {K, o, o, v}), S1v = mv(S1, {K, o}), YSv = mv(YS, {K, v + o}),
                XUv = mv(XU, {K, v + o}), Zv = mv(Z, {K, v, v, v});
    const TView LooV = mv(Loo, {o, o}), LvvV = mv(Lvv, {v, v}), T4 = mv(T, {v, v, o, o});
    // the ring-type terms: s2[j,i,a] += PA[(i,a),(l,d)] r2[j,l,d] + PB[(i,a),(l,d)] r2[l,j,d];  s2[j,i,a] += MDU[(j,a),(l,d)] r2[l,i,d]
    q.C(1.0, Rv, "zjld", mv(PA, {o, v, o, v}), "iald", 0.0, Dv, "zjia");
    q.C(1.0, Rxv, "zjld", mv(PB, {o, v, o, v}), "iald", 1.0, Dv, "zjia");
    q.C(1.0, Rxv, "zild", mv(MDU, {o, v, o, v}), "jald", 0.0, Ev, "zija");
    // Y_c = -V_lkcd (2 r2[l,k,d] - r2[k,l,d]) and the singles term -V_ijka[j,k,i,b] Rt[j,k,b] from one pass over Rt
    q.C(1.0, Rtv, "zlkd", mv(BB, {o, o, v, v + o}), "lkdn", 0.0, YSv, "zn");
    q.C(1.0, Rtv, "zijb", mv(fov, {o, v}), "jb", 0.0, S1v, "zi");
    q.C(-1.0, U1v, "zk", LooV, "ki", 1.0, S1v, "zi");
    e.axpby(1.0, slice(YSv, 1, v, v + o), 1.0, S1v);
    // one-index dressings and the hole ladder
    q.C(-1.0, LooV, "li", Rv, "zljb", 1.0, Dv, "zijb", "z");
    q.C(-1.0, LooV, "lj", Rv, "zilb", 1.0, Dv, "zijb", "zi");
    q.C(1.0, Rv, "zijd", LvvV, "bd", 1.0, Dv, "zijb");
    q.C(1.0, mv(B2, {o, o, o, o}), "klij", Rv, "zklb", 1.0, Dv, "zijb", "z");
    // D += [Y | r1] . [t ; A]
    e.copy(slice(YSv, 1, 0, v), slice(XUv, 1, 0, v));
    e.copy(U1v, slice(XUv, 1, v, v + o));
    q.C(1.0, XUv, "zn", mv(TA, {v + o, o, o, v}), "nijb", 1.0, Dv, "zijb");
    // -V_lacd t_cdji r1_l on the fly: (sum_l r1_l V_lacd) . t — no o^3 v block of it is stored
    q.C(1.0, U1v, "zl", V("iabc"), "lacd", 0.0, Zv, "zacd");
    q.C(-1.0, Zv, "zacd", T4, "cdji", 1.0, Ev, "zija");
    dev::ipea_assemble(k, D, E, nullptr, S1, no, nv, no, s1, s2, e.stream);
}

void IpEaSigma::apply_ea(int k, const double* const* r1, const double* const* r2, double* const* s1, double* const* s2) {
    const int64_t o = no, v = nv, K = k, n2 = v * v * o;
    const Ops q{e};
    Tmp U1(*this, K * v), R(*this, K * n2), Rx(*this, K * n2), Rt(*this, K * n2), Rn(*this, K * n2), D(*this, K * n2),
        E(*this, K * n2), L(*this, K * n2), S1(*this, K * v), XX(*this, K * o * o * o), yy(*this, K * o), Q(*this, K * o * v * v),
        Qp(*this, K * o * v * v);
    dev::ipea_pack(k, r1, r2, nv, no, nv, U1, R, Rx, Rt, Rn, e.stream);
    const TView U1v = mv(U1, {K, v}), Rv = mv(R, {K, v, v, o}), Rxv = mv(Rx, {K, v, v, o}), Rtv = mv(Rt, {K, v, v, o}),
                Dv = mv(D, {K, v, v, o}), Ev = mv(E, {K, v, v, o}), S1v = mv(S1, {K, v}), XXv = mv(XX, {K, o, o, o}),
                yyv = mv(yy, {K, o}), Qv = mv(Q, {K, o, v, v}), Qpv = mv(Qp, {o, v, v, K});
    const TView LooV = mv(Loo, {o, o}), LvvV = mv(Lvv, {v, v}), T4 = mv(T, {v, v, o, o}), FOV = mv(fov, {o, v});
    const TView Vijab = V("ijab"), Viabc = V("iabc");
    auto P4 = [&](double* p) { return mv(p, {v, o, v, o}); };
    // the ring-type terms: s2[b,a,i] += PA[(a,i),(d,l)] r2[b,d,l] + PB[(a,i),(d,l)] r2[d,b,l];  s2[b,a,i] += MDU[(b,i),(d,l)] r2[d,a,l]
    q.C(1.0, Rv, "zbdl", P4(PA), "aidl", 0.0, Dv, "zbai");
    q.C(1.0, Rxv, "zbdl", P4(PB), "aidl", 1.0, Dv, "zbai");
    q.C(1.0, Rxv, "zadl", P4(MDU), "bidl", 0.0, Ev, "zabi");
    // singles
    q.C(1.0, Rtv, "zabj", mv(fovT, {v, o}), "bj", 0.0, S1v, "za");
    q.C(1.0, U1v, "zb", LvvV, "ab", 1.0, S1v, "za");
    q.C(1.0, Viabc, "jabc", Rtv, "zcbj", 1.0, S1v, "za");
    // one-index dressings
    q.C(1.0, LvvV, "ad", Rv, "zdbj", 1.0, Dv, "zabj", "z");
    q.C(1.0, LvvV, "bc", Rv, "zacj", 1.0, Dv, "zabj", "za");
    q.C(-1.0, Rv, "zabk", LooV, "kj", 1.0, Dv, "zabj");
    // t[a,b,k,l] XX[k,l,j] + t[a,b,k,j] y_k:  XX = V_kldc r2[d,c,j] + V_ijka[l,k,j,d] r1_d,  y_k = -V_kldc Rt[d,c,l] - f_kd r1_d
    q.C(1.0, Vijab, "kldc", Rv, "zdcj", 0.0, XXv, "zklj", "z");
    q.C(1.0, V("ijka"), "lkjd", U1v, "zd", 1.0, XXv, "zklj");
    q.C(-1.0, Vijab, "kldc", Rtv, "zdcl", 0.0, yyv, "zk");
    q.C(-1.0, FOV, "kd", U1v, "zd", 1.0, yyv, "zk");
    q.C(1.0, T4, "abkl", XXv, "zklj", 1.0, Dv, "zabj", "z");
    q.C(1.0, T4, "abkj", yyv, "zk", 1.0, Dv, "zabj");
    // the V_kacd t r1 terms on the fly: Q[k,a,c] = V_kacd r1_d, Q'[k,a,c] = V_kadc r1_d — no v^3 o block of them is stored
    q.C(1.0, Viabc, "kacd", U1v, "zd", 0.0, Qv, "zkac");
    q.C(1.0, Viabc, "kadc", U1v, "zd", 0.0, Qpv, "kacz", "ka");
    q.C(1.0, Qv, "zkac", P4(TT), "ckbj", 1.0, Dv, "zabj");
    q.C(-1.0, Qpv, "kacz", P4(Td), "ckbj", 1.0, Dv, "zabj");
    q.C(-1.0, Qpv, "kbcz", P4(Tx), "ckaj", 1.0, Ev, "zbaj");
    q.C(1.0, V("abic"), "bajc", U1v, "zc", 1.0, Ev, "zbaj");
    // the particle ladder of all k vectors: ONE product over V_abcd, r2 in its natural [(c,d),(z,j)] layout
    q.C(1.0, V("abcd"), "abcd", mv(Rn, {v, v, K, o}), "cdzj", 0.0, mv(L, {v, v, K, o}), "abzj");
    dev::ipea_assemble(k, D, E, L, S1, nv, no, nv, s1, s2, e.stream);
}

// ---- the adjoint build (eom.h): each product of apply_ip / apply_ea once, trial-vector operand and output exchanged ----------------
void IpEaSigma::apply_left(int k, const double* const* l1, const double* const* l2, double* const* o1, double* const* o2) {
    if (k < 1) return;
    for (int z = 0; z < k; ++z)
        if (!l1[z] || !l2[z] || !o1[z] || !o2[z]) throw Error("ip/ea left sigma: null vector");
    const int step = stack_limit();
    for (int lo = 0; lo < k; lo += step) {
        const int g = std::min(k - lo, step);
        if (kind == IP) left_ip(g, l1 + lo, l2 + lo, o1 + lo, o2 + lo);
        else left_ea(g, l1 + lo, l2 + lo, o1 + lo, o2 + lo);
    }
}

void IpEaSigma::left_ip(int k, const double* const* l1, const double* const* l2, double* const* o1, double* const* o2) {
    const int64_t o = no, v = nv, K = k, n2 = o * o * v;
    const Ops q{e};
    // dS1, dD, dE: U1, R, Rx of the left vector (Rt of it is not read);  gU, gR, gX, gT: the derivatives with respect to U1, R, Rx, Rt
    Tmp dS1(*this, K * o), dD(*this, K * n2), dE(*this, K * n2), Ru(*this, K * n2), gU(*this, K * o), gR(*this, K * n2),
        gX(*this, K * n2), gT(*this, K * n2), dYS(*this, K * (v + o)), dXU(*this, K * (v + o)), dZ(*this, K * v * v * v);
    dev::ipea_pack(k, l1, l2, no, nv, no, dS1, dD, dE, Ru, nullptr, e.stream);
    const TView dS1v = mv(dS1, {K, o}), dDv = mv(dD, {K, o, o, v}), dEv = mv(dE, {K, o, o, v}), gUv = mv(gU, {K, o}),
                gRv = mv(gR, {K, o, o, v}), gXv = mv(gX, {K, o, o, v}), gTv = mv(gT, {K, o, o, v}), dYSv = mv(dYS, {K, v + o}),
                dXUv = mv(dXU, {K, v + o}), dZv = mv(dZ, {K, v, v, v});
    const TView LooV = mv(Loo, {o, o}), LvvV = mv(Lvv, {v, v}), T4 = mv(T, {v, v, o, o});
    // the ring-type terms
    q.C(1.0, dDv, "zjia", mv(PA, {o, v, o, v}), "iald", 0.0, gRv, "zjld");
    q.C(1.0, dDv, "zjia", mv(PB, {o, v, o, v}), "iald", 0.0, gXv, "zjld");
    q.C(1.0, dEv, "zija", mv(MDU, {o, v, o, v}), "jald", 1.0, gXv, "zild");
    // D += [Y | r1] . [t ; A] backwards, then dYS = [dXU_c | dS1] (the singles read YS_i directly)
    q.C(1.0, dDv, "zijb", mv(TA, {v + o, o, o, v}), "nijb", 0.0, dXUv, "zn");
    e.copy(slice(dXUv, 1, 0, v), slice(dYSv, 1, 0, v));
    e.copy(dS1v, slice(dYSv, 1, v, v + o));
    q.C(1.0, dYSv, "zn", mv(BB, {o, o, v, v + o}), "lkdn", 0.0, gTv, "zlkd");
    q.C(1.0, mv(dS1, {K, 1, o}), "zxi", mv(fov, {o, v, 1}), "jbx", 1.0, gTv, "zijb");
    q.C(-1.0, dS1v, "zi", LooV, "ki", 0.0, gUv, "zk");
    e.axpby(1.0, slice(dXUv, 1, v, v + o), 1.0, gUv);
    // one-index dressings and the hole ladder
    q.C(-1.0, LooV, "li", dDv, "zijb", 1.0, gRv, "zljb", "z");
    q.C(-1.0, LooV, "lj", dDv, "zijb", 1.0, gRv, "zilb", "zi");
    q.C(1.0, dDv, "zijb", LvvV, "bd", 1.0, gRv, "zijd");
    q.C(1.0, mv(B2, {o, o, o, o}), "klij", dDv, "zijb", 1.0, gRv, "zklb", "z");
    // -V_lacd t_cdji r1_l backwards: dZ = -dE . t, then against V_lacd read in place
    q.C(-1.0, dEv, "zija", T4, "cdji", 0.0, dZv, "zacd");
    q.C(1.0, dZv, "zacd", V("iabc"), "lacd", 1.0, gUv, "zl");
    dev::ipea_unpack(k, gU, gR, gX, gT, nullptr, no, nv, no, o1, o2, e.stream);
}

void IpEaSigma::left_ea(int k, const double* const* l1, const double* const* l2, double* const* o1, double* const* o2) {
    const int64_t o = no, v = nv, K = k, n2 = v * v * o;
    const Ops q{e};
    Tmp dS1(*this, K * v), dD(*this, K * n2), dE(*this, K * n2), Ru(*this, K * n2), dL(*this, K * n2), gU(*this, K * v),
        gR(*this, K * n2), gX(*this, K * n2), gT(*this, K * n2), gN(*this, K * n2), dXX(*this, K * o * o * o), dyy(*this, K * o),
        dQ(*this, K * o * v * v), dQp(*this, K * o * v * v);
    dev::ipea_pack(k, l1, l2, nv, no, nv, dS1, dD, dE, Ru, dL, e.stream);
    const TView dS1v = mv(dS1, {K, v}), dDv = mv(dD, {K, v, v, o}), dEv = mv(dE, {K, v, v, o}), gUv = mv(gU, {K, v}),
                gRv = mv(gR, {K, v, v, o}), gXv = mv(gX, {K, v, v, o}), gTv = mv(gT, {K, v, v, o}), dXXv = mv(dXX, {K, o, o, o}),
                dyyv = mv(dyy, {K, o}), dQv = mv(dQ, {K, o, v, v}), dQpv = mv(dQp, {o, v, v, K});
    const TView LooV = mv(Loo, {o, o}), LvvV = mv(Lvv, {v, v}), T4 = mv(T, {v, v, o, o}), FOV = mv(fov, {o, v});
    const TView Vijab = V("ijab"), Viabc = V("iabc");
    auto P4 = [&](double* p) { return mv(p, {v, o, v, o}); };
    // the ring-type terms
    q.C(1.0, dDv, "zbai", P4(PA), "aidl", 0.0, gRv, "zbdl");
    q.C(1.0, dDv, "zbai", P4(PB), "aidl", 0.0, gXv, "zbdl");
    q.C(1.0, dEv, "zabi", P4(MDU), "bidl", 1.0, gXv, "zadl");
    // singles
    q.C(1.0, mv(dS1, {K, 1, v}), "zxa", mv(fovT, {v, o, 1}), "bjx", 0.0, gTv, "zabj");
    q.C(1.0, dS1v, "za", LvvV, "ab", 0.0, gUv, "zb");
    q.C(1.0, Viabc, "jabc", dS1v, "za", 1.0, gTv, "zcbj");
    // one-index dressings
    q.C(1.0, LvvV, "ad", dDv, "zabj", 1.0, gRv, "zdbj", "z");
    q.C(1.0, LvvV, "bc", dDv, "zabj", 1.0, gRv, "zacj", "za");
    q.C(-1.0, dDv, "zabj", LooV, "kj", 1.0, gRv, "zabk");
    // t XX and t y backwards
    q.C(1.0, T4, "abkl", dDv, "zabj", 0.0, dXXv, "zklj", "z");
    q.C(1.0, T4, "abkj", dDv, "zabj", 0.0, dyyv, "zk");
    q.C(1.0, Vijab, "kldc", dXXv, "zklj", 1.0, gRv, "zdcj", "z");
    q.C(1.0, V("ijka"), "lkjd", dXXv, "zklj", 1.0, gUv, "zd");
    q.C(-1.0, Vijab, "kldc", dyyv, "zk", 1.0, gTv, "zdcl");
    q.C(-1.0, FOV, "kd", dyyv, "zk", 1.0, gUv, "zd");
    // the V_kacd t r1 terms backwards: dQ, dQ' of o v^2 per vector, then against V_kacd read in place
    q.C(1.0, dDv, "zabj", P4(TT), "ckbj", 0.0, dQv, "zkac");
    q.C(-1.0, dDv, "zabj", P4(Td), "ckbj", 0.0, dQpv, "kacz");
    q.C(-1.0, dEv, "zbaj", P4(Tx), "ckaj", 1.0, dQpv, "kbcz");
    q.C(1.0, Viabc, "kacd", dQv, "zkac", 1.0, gUv, "zd");
    q.C(1.0, Viabc, "kadc", dQpv, "kacz", 1.0, gUv, "zd");
    q.C(1.0, V("abic"), "bajc", dEv, "zbaj", 1.0, gUv, "zc");
    // the particle ladder of all k vectors backwards: ONE product over V_abcd
    q.C(1.0, V("abcd"), "abcd", mv(dL, {v, v, K, o}), "abzj", 0.0, mv(gN, {v, v, K, o}), "cdzj");
    dev::ipea_unpack(k, gU, gR, gX, gT, gN, nv, no, nv, o1, o2, e.stream);
}

void IpEaSigma::diagonals(double* d1, double* d2) {
    if (!d1 || !d2) throw Error("ip/ea diagonals: null argument");
    dev::ipea_diagonals(Loo, Lvv, kind == EA ? 1 : 0, no, nv, d1, d2, e.stream);
}

void IpEaSigma::correction(int n, const double* const* s, const double* const* r, const double* w_host, const double* d,
                           double shift, double* const* q, int64_t off2, int64_t len, double* norms_host) {
    if (n < 1) return;
    if (!s || !r || !w_host || !d || !q || !norms_host) throw Error("ip/ea correction: null argument");
    if (off2 < n1() || len != off2 + n2()) throw Error("ip/ea correction: the flat layout does not match the operator");
    for (int z = 0; z < n; ++z)
        if (!s[z] || !r[z] || !q[z]) throw Error("ip/ea correction: null vector");
    davidson_correction(e, n, s, r, w_host, d, shift, q, n1(), off2, len, norms_host);
}

// ---- Dyson amplitudes (eom.h; formulas in include/pymes_amd.h, pymes_ipea_dyson) ------------------------------------------------------
void ipea_dyson(Engine& e, IpEaSigma::Kind kind, const double* t1, const double* t2, const double* lam1, const double* lam2, int k,
                const double* const* l1, const double* const* l2, const double* const* r1, const double* const* r2,
                double* psiL_host, double* psiR_host) {
    if (!t1 || !t2 || !lam1 || !lam2 || !l1 || !l2 || !r1 || !r2 || !psiL_host || !psiR_host) throw Error("ipea_dyson: null argument");
    if (k < 1) throw Error("ipea_dyson: needs at least one root");
    for (int z = 0; z < k; ++z)
        if (!l1[z] || !l2[z] || !r1[z] || !r2[z]) throw Error("ipea_dyson: null vector");
    const bool ip = kind == IpEaSigma::IP;
    const int64_t o = e.no, v = e.nv, n = o + v, P = ip ? o : v, S = ip ? v : o, m = S, n2 = P * P * S;
    struct Buf {
        Engine& e;
        double* p;
        Buf(Engine& e_, int64_t d) : e(e_), p(e_.scratch_get(std::max<int64_t>(d, 1))) {}
        ~Buf() { e.scratch_put(p); }
    };
    const TView T4 = mv(t2, {v, v, o, o}), LAM1 = mv(lam1, {v, o}), LAM2 = mv(lam2, {v, v, o, o});
    // lambda . t, once per call
    Buf Yoo(e, o * o), Yvv(e, v * v);
    e.contract(1.0, LAM2, "abij", T4, "abkj", 0.0, mv(Yoo.p, {o, o}), "ki");
    e.contract(1.0, LAM2, "abij", T4, "cbij", 0.0, mv(Yvv.p, {v, v}), "ac");
    for (int lo = 0; lo < k; lo += 16) {
        const int g = std::min(16, k - lo);
        const int64_t K = g;
        Buf L1(e, K * P), R1(e, K * P), Lr(e, K * n2), Rr(e, K * n2), Xx(e, K * n2), Rt(e, K * n2), A(e, K * m), B(e, K * m),
            Cc(e, K * P), G(e, 2 * K * n);
        dev::ipea_pack(g, l1 + lo, l2 + lo, (int)P, (int)S, (int)P, L1.p, Lr.p, Xx.p, Rt.p, nullptr, e.stream);
        dev::ipea_pack(g, r1 + lo, r2 + lo, (int)P, (int)S, (int)P, R1.p, Rr.p, Xx.p, Rt.p, nullptr, e.stream);
        const TView Am = mv(A.p, {K, m}), Bm = mv(B.p, {K, m}), Cm = mv(Cc.p, {K, P});
        if (ip) {
            e.contract(1.0, mv(Rr.p, {K, o, o, v}), "zijb", LAM2, "abij", 0.0, Am, "za");
            e.contract(1.0, mv(Lr.p, {K, o, o, v}), "zijb", T4, "abij", 0.0, Bm, "za");
            e.contract(1.0, mv(Rt.p, {K, o, o, v}), "zjia", LAM1, "ai", 0.0, Cm, "zj");
        } else {
            e.contract(1.0, mv(Rr.p, {K, v, v, o}), "zabj", LAM2, "abij", 0.0, Am, "zi");
            e.contract(1.0, mv(Lr.p, {K, v, v, o}), "zabj", T4, "abkj", 0.0, Bm, "zk");
            e.contract(1.0, mv(Rt.p, {K, v, v, o}), "zbai", LAM1, "ai", 0.0, Cm, "zb");
        }
        dev::DysonParts q;
        q.t1 = t1; q.lam1 = lam1; q.Yoo = Yoo.p; q.Yvv = Yvv.p; q.L1 = L1.p; q.R1 = R1.p; q.A = A.p; q.B = B.p; q.C = Cc.p;
        q.psiL = G.p; q.psiR = G.p + K * n;
        dev::ipea_dyson_assemble(q, g, ip ? 0 : 1, e.no, e.nv, e.stream);
        dev::memcpy_d2h(psiL_host + lo * n, q.psiL, sizeof(double) * K * n, e.stream);
        dev::memcpy_d2h(psiR_host + lo * n, q.psiR, sizeof(double) * K * n, e.stream);
        dev::stream_sync(e.stream);
    }
}

}  // namespace pymes
