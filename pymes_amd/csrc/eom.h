// EOM-CCSD sigma build (pymes/solver/eom_ccsd.py:268-385) on the engine: the u-independent V.T intermediates hoisted once
// per solve (prepare), then H-bar . u for one trial vector or k stacked ones (apply), and the two diagonals
// (eom_ccsd.py:169-266).  The whole-step entry the boundary contract of SURVEY 8(b) names: eom_sigma(ctx, f~, u1, u2, T2).
#pragma once
#include <cstdint>
#include <map>
#include <vector>

#include "engine.h"

namespace pymes {

class EomSigma {
  public:
    // f_host: the T1-dressed Fock matrix [n,n] (host); t2: the CCSD doubles [v,v,o,o] (device; must outlive the object);
    // dressed: read the engine's T1-DRESSED blocks (dress_V) instead of the blocks as uploaded
    EomSigma(Engine& eng, const double* f_host, const double* t2, bool dressed);
    ~EomSigma();
    EomSigma(const EomSigma&) = delete;
    EomSigma& operator=(const EomSigma&) = delete;

    // bit 0: V_abcd = V_badc, 1: T_abij = T_baji, 2: the hole-ladder-shaped terms may run pair-packed, 3: fused pair kernels
    // available for this nocc, 4: the stacked multi-vector build is available (all of the above)
    int flags() const;
    // sigma for k trial vectors: s1[z] [v,o], s2[z] [v,v,o,o] (device, written).  sym[z] != 0: the caller knows that
    // u2[z]_abij = u2[z]_baji; sym == nullptr: tested here (one reduction and a synchronisation per vector)
    void apply(int k, const double* const* u1, const double* const* u2, const int* sym, double* const* s1, double* const* s2);
    bool exchange_symmetric(const double* x, int64_t d0, int64_t d2) const;
    Engine& engine() { return e; }
    void trim();                      // release the pooled temporaries

    // ---- the adjoint build: o = A^T l for the sigma A of apply() under the plain inner product over both arrays, on
    // the exchange-symmetric subspace, from the SAME hoisted intermediates read through transposed operand views.  l2[z] must
    // have the exchange symmetry (sym[z] != 0: the caller knows; else tested here, one reduction and a synchronisation; refused
    // by name otherwise).  The k vectors go through every product stacked (left_build: one GEMM per large product); k = 1 is a
    // stack of one, read in place.  apply() is not affected: nothing it reads is written.
    void apply_left(int k, const double* const* l1, const double* const* l2, const int* sym, double* const* o1,
                    double* const* o2);
    // One Lambda iteration for eta1[a,i] = 2 f_ov[i,a], eta2[a,b,i,j] = 2 V_ijab[i,j,a,b] - V_ijab[i,j,b,a] (read from the block):
    //   res = eta + A^T lam;  out = lam - res / d;  err = -err_scale res / d;  returns |res| (one synchronisation)
    // d1 = ev[a] - eo[i] - shift, d2 = ev[a] + ev[b] - eo[i] - eo[j] - shift (eo, ev on the host).  start: lam is taken as zero
    // and not read (out = -eta / d, the start vector; |eta| is returned); lam1 / lam2 may then be null.  known_sym: the caller
    // knows that lam2_abij = lam2_baji (the output of an earlier step, or a combination of such); else tested here.
    double lambda_step(const double* lam1, const double* lam2, const double* eo_host, const double* ev_host, double shift,
                       double err_scale, bool start, bool known_sym, double* out1, double* out2, double* err1, double* err2);

  private:
    Engine& e;
    const int no, nv;
    const bool dressed;
    const double* T;
    std::vector<double*> owned_;      // hoisted intermediates (engine scratch), returned by the destructor
    double* get(int64_t doubles);
    void put(double* p);
    double* keep(int64_t doubles);
    struct Tmp;                       // RAII temporary from the pool
    // hoisted quantities (names as pymes_amd/solver/eom_ccsd.py round 4, which this replaces)
    double *foo = nullptr, *fov = nullptr, *fvv = nullptr, *fovT = nullptr;
    double *Td = nullptr, *Tx = nullptr, *W1 = nullptr, *Gvv_s = nullptr, *Goo_s = nullptr, *M_C = nullptr, *M_D = nullptr,
           *M1 = nullptr, *Ud = nullptr, *M2 = nullptr, *M12 = nullptr, *MDU = nullptr, *WA = nullptr, *W3 = nullptr, *A3 = nullptr,
           *A4 = nullptr, *A6 = nullptr, *Gvv = nullptr, *Goo = nullptr, *B2 = nullptr, *L = nullptr, *WW = nullptr, *BB = nullptr,
           *Aoo = nullptr, *A346 = nullptr, *TA = nullptr, *LK3 = nullptr, *LK2 = nullptr;
    // the adjoint build: eta1, once per handle on first use; the partial results of one vector
    double *eta1 = nullptr, *eps_dev = nullptr;
    std::vector<double> eps_host_;
    bool left_ready = false;
    void left_check() const;
    void left_prepare();
    struct LeftBuild;                 // the partial results of K vectors and their K descriptions for the assembly
    void left_build(const double* const* l1, const double* const* l2, LeftBuild& w);
    void general_operands();          // LK3, LK2 (trial vectors without exchange symmetry), on first use
    bool v_sym = false, t_sym = false, hole_sym = false, fused_ok = false, many_ok = false;
    TView V(const char* name) const;
    void singles(const double* u1, const double* u2, double* s1);
    void doubles(const double* u1, const double* u2, bool u2_sym, double* s2, bool defer_ladder = false);
    void general_ladders(int g, const double* const* u2, double* const* s2);
    void stack(int k, const double* const* u1, const double* const* u2, double* const* s1, double* const* s2);
    int stack_limit() const;
};

// eom_ccsd.py:169-198 (get_diag_singles) / :200-266 (get_diag_doubles): d1 [v,o], d2 [v,v,o,o] (device, written); f_host the
// dressed Fock matrix [n,n], t2 [v,v,o,o] on the device, blocks read dressed or as set
void eom_diagonals(Engine& e, const double* f_host, const double* t2, bool dressed, double* d1, double* d2);

// The one-particle response density of the CCSD Lagrangian (formulas in include/pymes_amd.h, pymes_rdm1): gamma_host
// [n,n], occupied orbitals first, from t1, lam1 [v,o] and t2, lam2 [v,v,o,o] on the device; ref is added on the occupied
// diagonal (2.0: the matrix whose trace is the electron count).  Reads no integral block.
void lambda_rdm1(Engine& e, const double* t1, const double* t2, const double* lam1, const double* lam2, double ref,
                 double* gamma_host);

// The two-particle response density of the same Lagrangian (formulas in include/pymes_amd.h, pymes_rdm2):
// Gamma_pqrs = (G_pqrs + G_qpsr) / 2 with G = dL/dV at fixed f, so that L(f, V) = sum gamma f + sum Gamma V for every V with
// V_pqrs = V_qpsr.  Block by block: out[pattern] (device, written) for every pattern in `mask` (bit = the pattern number of
// pattern_of_name).  A block and its image under (pq,rs) -> (qp,sr) are the same data; rdm2_stored(pattern) names the one of
// each pair that can be asked for (klij, ijka, ijab, iajk, iajb, iabj, iabc, abij, abic, abcd).  Reads no integral block; t2 and
// lam2 must have the exchange symmetry; refused by name beyond PYMES_NOCC_MAX_LAMBDA.  abcd (v^4) is built only when asked for.
bool rdm2_stored(int pattern);
void lambda_rdm2(Engine& e, const double* t1, const double* t2, const double* lam1, const double* lam2, unsigned mask,
                 double* const out[16]);
// sum Gamma_pqrs W_pqrs over all sixteen blocks for the operator W held as the context's undressed blocks (W_pqrs = W_qpsr is
// tested and refused by name otherwise).  The abcd density is never built: its part is sum l2_abij (W_abcd tau_cdij) through the
// pair-packed ladder.  Deterministic: block sums in a fixed tree, added in order.  One synchronisation.
double lambda_rdm2_expectation(Engine& e, const double* t1, const double* t2, const double* lam1, const double* lam2);

// The transition densities of k EE-EOM-CCSD roots (formulas in include/pymes_amd.h, pymes_tdm1): gammaL, gammaR
// [k,n,n] and r0 [k] on the host from t1, lam1 [v,o], t2, lam2 [v,v,o,o] and the left / right vectors (l1[z], l2[z]), (r1[z],
// r2[z]) on the device.  Linear in every vector: normalisation is the caller's.  Reads no integral block.
void transition_densities(Engine& e, const double* t1, const double* t2, const double* lam1, const double* lam2, int k,
                          const double* const* l1, const double* const* l2, const double* const* r1, const double* const* r2,
                          double* gl_host, double* gr_host, double* r0_host);

// The property vectors of k <= 64 one-body operators for the EOM-CCSD linear response function (definitions and
// written-out formulas in include/pymes_amd.h, pymes_response_vectors): xi(O_z) = (R1(O_z), R2(O_z)) and the left vector
// eta(O_z) into the device arrays xi1[z], eta1[z] [v,o] and xi2[z], eta2[z] [v,v,o,o], g0_host[z] = <lambda, xi(O_z)>.
// ops_host [k,n,n] (occupied orbitals first, undressed: the T1 dressing is done here).  The contracted intermediates are engine
// products with the k operators stacked; the singles and g0 are one launch, the doubles one launch each for xi2 and eta2.  Reads
// no integral block; refuses (by name) t2 or lam2 without the exchange symmetry and outputs that alias inputs or each other.
void response_vectors(Engine& e, const double* t1, const double* t2, const double* lam1, const double* lam2, int k,
                      const double* ops_host, double* const* xi1, double* const* xi2, double* const* eta1, double* const* eta2,
                      double* g0_host);
// One sweep's arithmetic for n linear systems (z_s - A) x_s = xi_s over flat vectors (device_api.h, ResponseSystem; the
// pointers of `sys` are device vectors of `len` doubles, the rest host values).  response_dots: the dots of the orthogonalisation
// into dots_host [n, kResponseDots]; response_update: the fused step into norms_host [n] = |r_s|^2.  One launch pair and ONE
// synchronisation each, whatever n.
void response_dots(Engine& e, int n, const dev::ResponseSystem* sys, int64_t n1, int64_t off2, int64_t len, double* dots_host);
void response_update(Engine& e, int n, const dev::ResponseSystem* sys, const double* d, double floor, int64_t n1, int64_t off2,
                     int64_t len, double* norms_host);

// For n roots over flat vectors of `len` doubles ([0,n1) singles, [n1,off2) zero pad, [off2,len) doubles; d the diagonal in the
// same layout): q_n = (s_n - w_n r_n) / (w_n - d + shift) written (zero in the pad), norms[2 n] = |s_n - w_n r_n|^2,
// norms[2 n + 1] = |r_n|^2 (one launch and one synchronisation per sixteen roots, fixed summation order).  The kernel of the
// IP / EA driver; the EE drivers (right and left) use it with the diagonals of eom_diagonals.
void davidson_correction(Engine& e, int n, const double* const* s, const double* const* r, const double* w_host, const double* d,
                         double shift, double* const* q, int64_t n1, int64_t off2, int64_t len, double* norms_host);

// IP- and EA-EOM-CCSD sigma builds (formulas in include/pymes_amd.h): the EE operator above restricted to the sector
// with one non-interacting orbital.  Vectors: IP r1[i], r2[i,j,b]; EA r1[a], r2[a,b,j] — below r2[x,y,w] with x, y over P
// (no for IP, nv for EA) and w over S (nv for IP, no for EA).  Same life cycle as EomSigma: the constructor hoists what does
// not depend on the trial vector, apply() builds sigma for k stacked vectors (every hoisted operand and every integral block
// read once per call), diagonals() fills the preconditioner, correction() the Davidson expansion vectors of all roots.
class IpEaSigma {
  public:
    enum Kind { IP = 0, EA = 1 };
    // f_host: the T1-dressed Fock matrix [n,n] (host); t2: the CCSD doubles [v,v,o,o] (device; must outlive the object).
    // Throws, naming the symmetry, unless V_pqrs = V_qpsr on the blocks read and T_abij = T_baji.
    IpEaSigma(Engine& eng, Kind kind, const double* f_host, const double* t2, bool dressed);
    ~IpEaSigma();
    IpEaSigma(const IpEaSigma&) = delete;
    IpEaSigma& operator=(const IpEaSigma&) = delete;

    // the names of the dressed blocks the operator reads
    static const std::vector<const char*>& blocks(Kind kind);
    // bit 0: kind (0 IP, 1 EA); bit 1: the blocks are read dressed
    int flags() const { return (kind == EA ? 1 : 0) | (dressed ? 2 : 0); }
    int64_t n1() const { return kind == IP ? no : nv; }
    int64_t n2() const { return kind == IP ? static_cast<int64_t>(no) * no * nv : static_cast<int64_t>(nv) * nv * no; }
    // sigma for k trial vectors (device arrays): s1[z] [n1], s2[z] [n2] written
    void apply(int k, const double* const* r1, const double* const* r2, double* const* s1, double* const* s2);
    // The adjoint build: o = H^T l for the sigma H of apply() under the plain inner product over the compact vectors,
    // k stacked vectors per call under the same stack_limit().  ipea_pack of the left vector IS the adjoint of the assembly (R, Rx,
    // Rn, U1 of l are the derivatives with respect to D, E, L, S1); every product of apply_ip / apply_ea then runs once with its
    // trial-vector operand and its output exchanged, from the same hoisted operands and the same blocks read in place; ipea_unpack
    // (the adjoint of the packing) adds the four partial results.  apply() is not affected: nothing it reads is written.
    void apply_left(int k, const double* const* l1, const double* const* l2, double* const* o1, double* const* o2);
    // d1 [n1] = -L_ii (IP) / L_aa (EA); d2 [n2] = L_bb - L_ii - L_jj (IP) / L_aa + L_bb - L_jj (EA): the dressed one-body part
    void diagonals(double* d1, double* d2);
    // For n roots (flat vectors of `len` doubles: [r1 (n1) | zero pad | r2 (n2)], the doubles part at `off2`; d the flat
    // diagonals in the same layout): q_n = (s_n - w_n r_n) / (w_n - d + shift) written (zero in the pad) and
    // norms[2 n] = |s_n - w_n r_n|^2, norms[2 n + 1] = |r_n|^2 returned (one synchronisation, fixed summation order)
    void correction(int n, const double* const* s, const double* const* r, const double* w_host, const double* d, double shift,
                    double* const* q, int64_t off2, int64_t len, double* norms_host);
    Engine& engine() { return e; }
    Kind which() const { return kind; }
    const double* amplitudes() const { return T; }
    void trim() { e.scratch_trim(); }

  private:
    Engine& e;
    const Kind kind;
    const int no, nv;
    const bool dressed;
    const double* T;
    std::vector<double*> owned_;
    double* keep(int64_t doubles);
    struct Tmp;
    TView V(const char* name) const;
    void hoist(const double* f_host);
    void apply_ip(int k, const double* const* r1, const double* const* r2, double* const* s1, double* const* s2);
    void apply_ea(int k, const double* const* r1, const double* const* r2, double* const* s1, double* const* s2);
    void left_ip(int k, const double* const* l1, const double* const* l2, double* const* o1, double* const* o2);
    void left_ea(int k, const double* const* l1, const double* const* l2, double* const* o1, double* const* o2);
    int stack_limit() const;
    // hoisted: L_oo [o,o], L_vv [v,v], f_ov [o,v] and its transpose; the (ov) x (ov) pair matrices PA = 2 M1 + M2,
    // PB = M_C - M1, MDU = M_D - U (names of EomSigma), pair index (a,i) for EA and (i,a) for IP; IP: W_klij, TA [(c | l),i,j,b],
    // BB [(l,k,d),(c | i)]; EA: the pair layouts of T
    double *Loo = nullptr, *Lvv = nullptr, *fov = nullptr, *fovT = nullptr, *PA = nullptr, *PB = nullptr, *MDU = nullptr,
           *B2 = nullptr, *TA = nullptr, *BB = nullptr, *TT = nullptr, *Td = nullptr, *Tx = nullptr;
};

// The Dyson amplitudes of k IP / EA roots (definitions and written-out formulas in include/pymes_amd.h,
// pymes_ipea_dyson): psiL_host, psiR_host [k,n] (occupied orbitals first) from t1, lam1 [v,o], t2, lam2 [v,v,o,o] and the left /
// right vectors (l1[z], l2[z]), (r1[z], r2[z]) on the device (compact: IP [o], [o,o,v]; EA [v], [v,v,o]).  Linear in every vector:
// normalisation is the caller's.  Reads no integral block.
void ipea_dyson(Engine& e, IpEaSigma::Kind kind, const double* t1, const double* t2, const double* lam1, const double* lam2, int k,
                const double* const* l1, const double* const* l2, const double* const* r1, const double* const* r2,
                double* psiL_host, double* psiR_host);

}  // namespace pymes
