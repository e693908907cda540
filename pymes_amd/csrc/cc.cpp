// Coupled-cluster term sequences on top of Engine::contract / permute.
//
// Every function cites the reference lines it reproduces (nickirk/pymes @ 2024_10_08).
// The index algebra is restated for GEMM-friendly layouts; no symmetry of V or T is
// assumed anywhere (the transcorrelated Hamiltonian has only V_pqrs = V_qpsr, and the
// reference keeps V_ijab and V_abij separate, ccd.py:172).
//
// Matrix layouts used for the o^3 v^3 terms (all ov x ov matrices):
//   Td[(a,i),(b,j)] = T[a,b,i,j]   "direct" pairing      (labels "aibj")
//   Tx[(a,j),(b,i)] = T[a,b,i,j]   "crossed" pairing     (labels "ajbi")
// so that every ring/exchange term of ccd.py:190-240 is a plain product of two such
// matrices (possibly transposed), with no per-term transposition of the operands.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <cstdlib>
#include <optional>
#include <vector>

#include "../../include/pymes_amd.h"
#include "engine.h"

#include <cmath>

namespace pymes {
static_assert(Engine::kT1Zero == PYMES_T1_ZERO && Engine::kOwnerTiles == PYMES_OWNER_TILES,
              "the engine's flag bits are the public ones");

namespace {
// `rows` rows of pair-packed integrals V^+- at their pitch (PairDims::lpitch), `cols` of them defined
inline int64_t lpitch(int64_t n) { return PairDims::lpitch(n); }
inline TView packed_rows(double* p, int64_t rows, int64_t cols) { return slice(make_view(p, {rows, lpitch(cols)}), 1, 0, cols); }
// r rows of pitch ld, the first c columns of each
inline TView pitched(double* p, int64_t r, int64_t c, int64_t ld) { return slice(make_view(p, {r, ld}), 1, 0, c); }
constexpr int P_klij = 0, P_ijka = 1, P_ijak = 2, P_ijab = 3, P_iajk = 4, P_iajb = 5, P_iabj = 6, P_iabc = 7,
              P_aibc = 11, P_abij = 12, P_abic = 13, P_abci = 14, P_abcd = 15;
}

// -----------------------------------------------------------------------------------
// static (per-solve) permutations of the undressed V_ijab block.  The T1-dressed ijab
// block is a plain copy of the undressed one (ccsd.py:355-357), so these stay valid for
// the whole solve.
// -----------------------------------------------------------------------------------
double* Engine::get_static(const std::string& key) {
    auto it = static_.find(key);
    if (it != static_.end()) return it->second;
    const int64_t o = no, v = nv;
    TView Vijab = block(P_ijab);
    double* p = new_static(key, o * o * v * v);
    // all keys: source labels of V_ijab are "klcd" (k,l occupied; c,d virtual)
    if (key == "Vd") permute(1.0, Vijab, "klcd", 0.0, make_view(p, {v, o, v, o}), "ckdl");        // [(c,k),(d,l)]
    else if (key == "Vx") permute(1.0, Vijab, "klcd", 0.0, make_view(p, {v, o, v, o}), "cldk");   // [(c,l),(d,k)]
    else if (key == "Ld") {                                      // 2 Vd - Vx: Ld[(c,k),(d,l)] = 2 V_klcd - V_lkcd
        permute(2.0, Vijab, "klcd", 0.0, make_view(p, {v, o, v, o}), "ckdl");
        permute(-1.0, Vijab, "lkcd", 1.0, make_view(p, {v, o, v, o}), "ckdl");
    }
    else if (key == "Ldh") {                                     // Ld / 2 = Vd - Vx / 2 (the D-term build of the paired ring products)
        permute(1.0, Vijab, "klcd", 0.0, make_view(p, {v, o, v, o}), "ckdl");
        permute(-0.5, Vijab, "lkcd", 1.0, make_view(p, {v, o, v, o}), "ckdl");
    }
    else if (key == "Vk") permute(1.0, Vijab, "lkdc", 0.0, make_view(p, {o, v, o, v}), "kdlc");   // [(k,d,l),c]
    else if (key == "Vk2") permute(1.0, Vijab, "lkdc", 0.0, make_view(p, {o, v, v, o}), "kcdl");  // [k,(c,d,l)]
    // K-major copies for the o x o results contracted over o v^2 (K = 2e6 at the benchmark size): with the long index
    // slowest both GEMM operands stream contiguously instead of gathering 128-byte pieces of 50 distant rows
    else if (key == "Vk3") permute(1.0, Vijab, "lkdc", 0.0, make_view(p, {v, v, o, o}), "cdlk");  // [(c,d,l),k]
    else if (key == "Vjbck") permute(1.0, Vijab, "kjbc", 0.0, make_view(p, {o, v, v, o}), "jbck"); // [(j,b,c),k]
    else if (key == "Edir") permute(1.0, Vijab, "ijab", 0.0, make_view(p, {v, v, o, o}), "abij"); // V[i,j,a,b]
    else if (key == "Eex") permute(1.0, Vijab, "ijba", 0.0, make_view(p, {v, v, o, o}), "abij");  // V[i,j,b,a]
    else throw Error("unknown static tensor " + key);
    return p;
}

// -----------------------------------------------------------------------------------
// mp2.py:9-22
// -----------------------------------------------------------------------------------
void Engine::mp2(double shift, double* t2, double e_out[2]) {
    const int64_t o = no, v = nv, n4 = v * v * o * o;
    need_eps("mp2");
    TView Vabij = block(P_abij);
    dev::mp2_amplitudes(t2, Vabij.p, eps_o, eps_v, shift, no, nv, stream);                 // :16-18
    ArenaScope scope(arena);
    double* e2 = arena.alloc(n4);
    permute(1.0, block(P_ijab), "jiab", 0.0, make_view(e2, {v, v, o, o}), "abij");          // 'abij,jiab' :20
    const double* x[2] = {t2, t2};
    const double* y[2] = {get_static("Edir"), e2};
    const int64_t len[2] = {n4, n4};
    double d[2];
    dev::dots(2, x, y, len, d, stream);
    e_out[0] = 2.0 * d[0];                                                                  // :19
    e_out[1] = -1.0 * d[1];                                                                 // :20
}

// -----------------------------------------------------------------------------------
// ccd.py:164-254  (the doubles residual; also the CCSD one via dressed blocks, ccsd.py:440-456)
// -----------------------------------------------------------------------------------
void Engine::doubles_residual(const double* f, const double* t2, double* r2, unsigned flags) {
    refuse_if_sharded("doubles_residual");
    const bool dcd = flags & PYMES_DCD, dressed = flags & PYMES_USE_DRESSED, skip_ladder = flags & PYMES_SKIP_LADDER,
               sym_ladder = flags & PYMES_SYM_LADDER, sym_rings = flags & PYMES_SYM_RINGS;
    // (factor-direct: the CCD / DCD loop runs here with the pair-packed undressed ladder; the forms that read V_abcd are refused)
    if (!skip_ladder && (!sym_ladder || dressed)) refuse_if_direct("doubles_residual with the full or dressed V_abcd");
    const bool quad = !dcd;
    const int64_t o = no, v = nv, nn = n;
    if (sym_rings) {      // symmetry-reduced evaluation = the one-rank case of the sharded form
        ArenaScope sc(arena);
        double* ETd = arena.alloc(o * v * o * v);
        double* ETx = arena.alloc(o * v * o * v);
        double* L = (sym_ladder && !skip_ladder) ? arena.alloc(v * (v + 1) / 2 * o * o) : nullptr;
        residual_slab(f, t2, ETd, ETx, L, 0, 1, flags);
        residual_finish(f, t2, ETd, ETx, L, r2, flags);
        return;
    }
    const double w = quad ? 1.0 : 0.5;                                                      // :213-220
    TView T = make_view(const_cast<double*>(t2), {v, v, o, o});
    TView R = make_view(r2, {v, v, o, o});
    TView F = make_view(const_cast<double*>(f), {nn, nn});
    TView Foo = slice(slice(F, 0, 0, o), 1, 0, o), Fvv = slice(slice(F, 0, o, nn), 1, o, nn);
    TView Vklij = block(P_klij, dressed), Vabij = block(P_abij, dressed), Viajb = block(P_iajb, dressed),
          Viabj = block(P_iabj, dressed);
    TView Vijab = block(P_ijab);   // dressed ijab == undressed ijab (ccsd.py:355-357)

    ArenaScope scope(arena);
    auto ov2 = [&]() { return make_view(arena.alloc(o * o * v * v), {v, o, v, o}); };
    TView Vd = make_view(get_static("Vd"), {v, o, v, o});
    TView Vk = make_view(get_static("Vk"), {o, v, o, v});
    TView Vk2 = make_view(get_static("Vk2"), {o, v, v, o});

    // permuted amplitudes: Td, Tx and Tt_d = direct layout of 2T - T^(ab)   (:199)
    TView Td = ov2(), Tx = ov2(), Ttd = ov2();
    permute(1.0, T, "abij", 0.0, Td, "aibj");
    permute(1.0, T, "abij", 0.0, Tx, "ajbi");
    permute(2.0, T, "abij", 0.0, Ttd, "aibj");
    permute(-1.0, T, "baij", 1.0, Ttd, "aibj");

    // ---- terms kept in the natural [a,b,i,j] layout -------------------------------------
    copy(Vabij, R);                                                                         // :185
    {
        ArenaScope s2(arena);
        TView hole = make_view(arena.alloc(o * o * o * o), {o, o, o, o});
        copy(Vklij, hole);                                                                  // :178
        if (quad) contract(1.0, Vijab, "klcd", T, "cdij", 1.0, hole, "klij");                // :180
        contract(1.0, hole, "klij", T, "abkl", 1.0, R, "abij");                             // :186
    }
    if (!skip_ladder) {                                                                     // :187
        if (sym_ladder) {
            ArenaScope s2(arena);
            double* L = arena.alloc(v * (v + 1) / 2 * o * o);
            ladder_sym(t2, L, 0, v * (v + 1) / 2, dressed, 0);
            ladder_sym_unpack(L, r2, 1.0);
        } else {
            contract(1.0, block(P_abcd, dressed), "abcd", T, "cdij", 1.0, R, "abij");
        }
    }

    // ---- X_ac, X_ki (:206-221) ------------------------------------------------------------
    TView Xvv = make_view(arena.alloc(v * v), {v, v}), Xoo = make_view(arena.alloc(o * o), {o, o});
    copy(Fvv, Xvv);
    copy(Foo, Xoo);
    // X_ac = f_ac - w sum_{dkl} Tt[a,d,k,l] V[l,k,d,c];  Tt[a,d,k,l] = Ttd[a,k,d,l]
    contract(-w, Ttd, "akdl", Vk, "kdlc", 1.0, Xvv, "ac");
    {
        // X_ki = f_ki + w sum_{cdl} Tt[c,d,i,l] V[l,k,d,c];  Tt[c,d,i,l] = Ttd[c,i,d,l]
        ArenaScope s2(arena);
        TView Tp = make_view(arena.alloc(o * o * v * v), {o, v, v, o});
        permute(1.0, Ttd, "cidl", 0.0, Tp, "icdl");
        contract(w, Vk2, "kcdl", Tp, "icdl", 1.0, Xoo, "ki");
    }

    // ---- accumulators in the pair layouts ---------------------------------------------------
    TView Exn = make_view(arena.alloc(o * o * v * v), {v, v, o, o});
    contract(1.0, Xvv, "ac", T, "cbij", 0.0, Exn, "abij");                                   // :231
    TView Exd = ov2(), Exx = ov2();
    TView Rd = ov2();
    {
        // :202-204  R += Tt . (V . Tt)   in the direct layout
        ArenaScope s2(arena);
        TView Y = ov2();
        contract(1.0, Vd, "ckdl", Ttd, "dlbj", 0.0, Y, "ckbj");
        contract(1.0, Ttd, "aick", Y, "ckbj", 0.0, Rd, "aibj");
    }
    {
        ArenaScope s2(arena);
        TView Ud = ov2(), Wd = ov2();
        permute(1.0, Viajb, "kaic", 0.0, Ud, "aick");     // Ud[(a,i),(c,k)] = V_iajb[k,a,i,c]
        permute(1.0, Viabj, "kbcj", 0.0, Wd, "ckbj");     // Wd[(c,k),(b,j)] = V_iabj[k,b,c,j]
        contract(-1.0, Ud, "aick", Td, "ckbj", 0.0, Exd, "aibj");                            // :233
        contract(1.0, Ttd, "aick", Wd, "ckbj", 1.0, Exd, "aibj");                            // :235
        contract(-1.0, Tx, "ajck", Ud, "bick", 0.0, Exx, "ajbi");                            // :234
    }
    contract(-1.0, Xoo, "ki", Td, "akbj", 1.0, Exd, "aibj", "a");                            // :232
    TView Rx;
    if (quad) {
        TView Vx = make_view(get_static("Vx"), {v, o, v, o});
        {
            // :238-240  Z[(a,i),(c,l)] = sum_{dk} T[d,a,k,i] V[k,l,c,d];  Ex += Z . (T[b,c,l,j] - T[c,b,l,j])
            ArenaScope s2(arena);
            TView Z = ov2(), Q = ov2();
            contract(1.0, Td, "dkai", Vx, "cldk", 0.0, Z, "aicl");
            permute(-1.0, T, "cblj", 0.0, Q, "clbj");
            permute(1.0, T, "bclj", 1.0, Q, "clbj");
            contract(1.0, Z, "aicl", Q, "clbj", 1.0, Exd, "aibj");
        }
        // :190-191  R += (Tx . Vx^T) . Tx   in the crossed layout
        Rx = ov2();
        TView X1 = ov2();
        contract(1.0, Tx, "ajdk", Vx, "cldk", 0.0, X1, "ajcl");
        contract(1.0, X1, "ajcl", Tx, "clbi", 0.0, Rx, "ajbi");
    }

    // ---- assemble: R += P(Rd) + P(Rx) + Ex + Ex^T(1,0,3,2)   (:249-252) ----------------------
    permute(1.0, Rd, "aibj", 1.0, R, "abij");
    if (quad) permute(1.0, Rx, "ajbi", 1.0, R, "abij");
    permute(1.0, Exd, "aibj", 1.0, R, "abij");
    permute(1.0, Exd, "bjai", 1.0, R, "abij");
    permute(1.0, Exx, "ajbi", 1.0, R, "abij");
    permute(1.0, Exx, "biaj", 1.0, R, "abij");
    permute(1.0, Exn, "abij", 1.0, R, "abij");
    permute(1.0, Exn, "baji", 1.0, R, "abij");
}

// -----------------------------------------------------------------------------------
// Symmetry-reduced, shardable T2 residual (requires T_abij = T_baji and V_pqrs = V_qpsr).
//
// Exchange-symmetric amplitudes make Td, Tx, Tt_d, Vd, Vx symmetric ov x ov matrices.  Round 1 merged the ten
// o^3v^3 products of the reference into 6 (5 -> 4 for DCSD) inside its own term structure; round 2 uses the C / D form of
// the closed-shell doubles equations, which is the same sum in 4 (3) products — see the comment at the products below:
//     Exd = 1/2 Tt_d (2 Wd - UdT + 1/2 Ld Tt_d) - 1/2 Xc,   Exx = -Xc,   Xc = Tx (UdT - 1/2 Vx Tx),   Ld = 2 Vd - Vx,
//     Wd[(c,k),(b,j)] = V_iabj[k,b,c,j],  UdT[(c,k),(b,j)] = V_iajb[k,b,j,c]
// COLUMNS (b,j) of these products never mix, so a rank needs no communication to compute its column
// slab; the slab is produced TRANSPOSED (ET[(b,j),(a,i)] = Ex[(a,i),(b,j)]) so that the slabs of all
// ranks are contiguous row blocks of ETd / ETx = one all-gather each.  Since only Ex + Ex^T enters R
// the transposition needs no undoing.  The pair-packed ladder rows of the same rank go to L.
// -----------------------------------------------------------------------------------
void Engine::ensure_xs() {
    if (!xs_oo_) xs_oo_ = static_cast<double*>(dev::dmalloc(sizeof(double) * no * no));
    if (!xs_vv_) xs_vv_ = static_cast<double*>(dev::dmalloc(sizeof(double) * nv * nv));
}

bool Engine::ring_fold_enabled() {
    if (const char* e = getenv("PYMES_RING_FOLD")) return atoi(e) != 0;
    return true;
}

// The three pair layouts of T2 (Td, Tx, Tt_d) in the engine's persistent buffers
bool Engine::sym_tail() const {
    if (const char* e = getenv("PYMES_SYM_TAIL"))
        if (atoi(e) == 0) return false;
    return dev::sym_tail_ok() && dev::fused_pair_kernels_ok(no);
}

void Engine::pair_layouts_of(const double* t2, bool want_td, bool sym) {
    const int64_t o = no, v = nv, ov = o * v;
    for (int i = want_td ? 0 : 1; i < 3; ++i)
        if (!lay_[i]) {
            if (capturing_) throw Error("pair_layouts_of: the pair layouts must exist before a launch graph is recorded (run one eager pass first)");
            lay_[i] = static_cast<double*>(dev::dmalloc(sizeof(double) * ov * ov));
        }
    lay_t2_ = nullptr;
    if (dev::fused_pair_kernels_ok(no)) {
        if (sym && sym_tail()) dev::t2_layouts_sym(t2, want_td ? lay_[0] : nullptr, lay_[1], lay_[2], no, nv, stream);
        else dev::t2_layouts(t2, want_td ? lay_[0] : nullptr, lay_[1], lay_[2], no, nv, stream);
        stats.permute_calls++;
        stats.permute_bytes += 8.0 * (want_td ? 5.0 : 4.0) * double(ov * ov);      // T twice, two or three layouts out
    } else {
        TView T = make_view(const_cast<double*>(t2), {v, v, o, o});
        TView t4 = make_view(lay_[0], {v, o, v, o});
        if (want_td) permute(1.0, T, "abij", 0.0, t4, "aibj");
        t4.p = lay_[1];
        permute(1.0, T, "abij", 0.0, t4, "ajbi");
        t4.p = lay_[2];
        permute(2.0, T, "abij", 0.0, t4, "aibj");
        permute(-1.0, T, "baij", 1.0, t4, "aibj");
    }
    lay_t2_ = t2;
}

// The three parts of residual_slab.  The ladder half: this rank's rows of the pair-packed ladders (and of QK with t1).
void Engine::slab_ladders(const double* t2, double* L, int rank, int world, unsigned flags, const double* t1, double* QK,
                          const double* P) {
    const bool dcd = flags & PYMES_DCD, dressed = flags & PYMES_USE_DRESSED;
    const int64_t o = no, v = nv;
    int64_t r0, r1;
    chunk(pair_dims().npp, rank, world, r0, r1);
    if (t1) {
        if (!QK) throw Error("residual_slab: QK buffer missing");
        int64_t q0, q1;
        chunk(o * v, rank, world, q0, q1);
        ladder_t1(t1, t2, L, r0, r1, QK, q0, q1, dcd, P ? P + o * o : nullptr);
    } else {
        ladder_sym(t2, L, r0, r1, dressed, dcd ? 2 : 1);   // particle AND hole ladder rows of this rank
    }
}

// The ring half of a rank that holds some of the columns.
void Engine::slab_rings_rows(const RingSlab& s) {
    const int64_t ov = static_cast<int64_t>(no) * nv, c0 = s.c0, c1 = s.c1, nc = c1 - c0;
    const bool quad = s.quad;
    const TView &Tx = s.Tx, &Ttd = s.Ttd, &ETd = s.ETd, &ETx = s.ETx;
    auto pairm = [&](double* p) { return make_view(p, {ov, ov}); };
    // Several ranks: the slab in its TRANSPOSED form from the start.  MT[(b,j),(c,k)] / N1T hold the rank's columns as
    // ROWS; Tt_d, Tx, Ld, Vx, Vd are symmetric pair matrices, so
    //     MT += rows(Tt_d) Ld / 2,  N1T += rows(Tx) Vx / 2,  ET_x = N1T Tx,  ET_d = MT Tt_d / 2 + ET_x / 2
    // are all products with a K-contiguous left and an N-contiguous right operand — the LDS-DMA variant that runs at 93 %
    // of peak on one rank (the column form needed the <false,true> variant for its applications: 85.5 % at N = 8,
    // profiles/r03/stub_rank0_of8.json) — and their outputs ARE the contiguous row blocks of ETd / ETx that are exchanged.
    auto slabT = [&]() { return make_view(arena.alloc(nc * ov), {nc, ov}); };
    TView MT = slabT(), N1T = slabT();
    s.load_rows(2.0, s.Viabj, "kbcj", MT);                                               // MT = (2 Wd)^T
    s.load_rows(-1.0, s.Viajb, "kbjc", N1T);                                             // N1T = -(UdT)^T
    axpby(1.0, N1T, 1.0, MT);
    ring_xd_ = 0.0;
    auto rowsOf = [&](const TView& m) { return slice(m, 0, c0, c1); };
    if (quad) {
        contract(0.5, rowsOf(Ttd), "ny", pairm(get_static("Ld")), "yx", 1.0, MT, "nx");
        contract(0.5, rowsOf(Tx), "ny", pairm(get_static("Vx")), "yx", 1.0, N1T, "nx");
    } else {
        contract(1.0, rowsOf(Ttd), "ny", pairm(get_static("Vd")), "yx", 1.0, MT, "nx");
    }
    contract(1.0, N1T, "nk", Tx, "km", 0.0, ETx, "nm");                                  // (Ex_x)^T, rows = this rank's columns
    contract(0.5, MT, "nk", Ttd, "km", 0.5, ETd, "nm", "", &ETx);                        // (Ex_d)^T
}

// The ring half of the one rank that holds all columns.
void Engine::slab_rings_cols(const RingSlab& s) {
    const int64_t o = no, v = nv, nn = n, ov = o * v, c0 = s.c0, c1 = s.c1, nc = c1 - c0;
    const bool quad = s.quad, traces = s.traces, fold = s.fold;
    const double w = quad ? 1.0 : 0.5;
    const double* t2 = s.t2;
    const TView &F = s.F, &Viajb = s.Viajb, &Viabj = s.Viabj, &Tx = s.Tx, &Ttd = s.Ttd, &ETd = s.ETd, &ETx = s.ETx;
    auto pairm = [&](double* p) { return make_view(p, {ov, ov}); };
    auto slab = [&]() { return make_view(arena.alloc(ov * nc), {ov, nc}); };
    auto cols = [&](const TView& m) { return slice(m, 1, c0, c1); };
    TView M = slab(), N1 = slab();
    // One rank with all columns: the two builds are independent, and so are the two applications once the D-term no longer
    // carries the half of the C-term (Ex_d = D + Ex_x / 2: the assembly reads Ex_x in both placements, `ring_xd_`) — each pair
    // is ONE batched launch of 2 x tiles (the second operand set addressed through pointer differences as batch strides).
    // At (20,80) a product is 169 tiles of 128 x 128 on 256 CUs, 3-way k-split with its reduction; a pair is 338 tiles:
    // 256 whole ones and an 82-tile tail.  M is kept halved (M_h = Wd - UdT / 2 + Ld Tt_d / 4) so that both products of a
    // pair share alpha.
    // Only where a single product under-fills the chip (< 512 tiles of 128 x 128): a big product loses nothing on its own,
    // and the assembly's two extra reads of Ex_x (1.6 GB at (50,200)) would be paid for nothing.
    const int64_t ring_tiles = ((ov + 127) / 128) * ((ov + 127) / 128);
    const bool paired = ring_tiles < 512;
    ring_xd_ = paired ? 0.5 : 0.0;
    auto pair_gemm = [&](double alpha, const double* A0, const double* A1, const double* B0, const double* B1, double beta,
                         double* C0, double* C1) {
        auto diff = [](const double* x, const double* y) {
            return static_cast<int64_t>((reinterpret_cast<intptr_t>(x) - reinterpret_cast<intptr_t>(y)) / 8);
        };
        dev::Gemm g{};
        g.M = ov; g.N = ov; g.K = ov; g.alpha = alpha; g.beta = beta;
        g.A = A0; g.a_sm = ov; g.a_sk = 1;          // symmetric pair matrices on the left, K-contiguous
        g.B = B0; g.b_sk = ov; g.b_sn = 1;
        g.C = C0; g.ldc = ov;
        g.nb1 = 2; g.nb2 = 1;
        g.a_b1 = diff(A1, A0); g.b_b1 = diff(B1, B0); g.c_b1 = diff(C1, C0);
        g.a_b2 = g.b_b2 = g.c_b2 = 0;
        g.splitk_ws = splitk_ws_;
        g.splitk_ws_doubles = splitk_doubles_;
        dev::gemm(g, stream);
        stats.gemm_calls++;
        stats.gemm_flops += 4.0 * double(ov) * double(ov) * double(ov);
    };
    auto dense = [](const TView& t) {
        int64_t st = 1;
        for (int i = t.rank - 1; i >= 0; --i) { if (t.st[i] != st) return false; st *= t.dim[i]; }
        return true;
    };
    if (dense(Viabj) && dense(Viajb) && (size_t)no * 33 * sizeof(double) <= 64 * 1024) {
        // both operands in one pass over the two blocks (two permutations and an axpby before: 5 reads / 3 writes of (ov)^2)
        dev::ring_operands(Viabj.p, Viajb.p, M.p, N1.p, paired ? 1.0 : 2.0, paired ? 0.5 : 1.0, no, nv, stream);
        stats.permute_calls++;
        stats.permute_bytes += 8.0 * 4.0 * double(ov) * double(ov);
    } else {
        s.load_cols(paired ? 1.0 : 2.0, Viabj, "kbcj", M);                                      // M = 2 Wd  (paired: Wd)
        s.load_cols(-1.0, Viajb, "kbjc", N1);                                                   // N1 = -UdT
        axpby(paired ? 0.5 : 1.0, N1, 1.0, M);                                               // M = 2 Wd - UdT  (paired: half of it)
    }
    // The small V.T sums S_ac = sum_dkl Tt_adkl V_lkdc, S_ki = sum_cdl Tt_cdil V_lkdc (X_ac, X_ki, ccsd.py:434 / :436) are
    // partial traces of the builds: tr(Vd Tt_d) for DCSD, (3 tr(Vx Tx) + tr(Ld Tt_d)) / 4 for CCSD — read off the
    // accumulators before and after the products (all columns on this rank only)
    const double cz = (quad ? 0.5 : 1.0) * (paired ? 2.0 : 1.0), cu = 1.5;   // (tr after - tr before) x these = the contribution to S
    if (traces) {
        ensure_xs();
        xs_oo_tag_.clear();
        xs_vv_tag_.clear();
        dev::pair_traces(M.p, nc, -cz, 0.0, xs_vv_, xs_oo_, no, nv, stream, quad ? N1.p : nullptr, -cu);
    }
    if (quad && paired) {
        pair_gemm(0.5, get_static("Ldh"), get_static("Vx"), Ttd.p, Tx.p, 1.0, M.p, N1.p);    // M_h += Ld Tt_d / 4, N1 += Vx Tx / 2
    } else if (quad) {
        contract(0.5, pairm(get_static("Ld")), "xy", cols(Ttd), "yn", 1.0, M, "xn");         // M = 2 Wd - UdT + Ld Tt_d / 2
        contract(0.5, pairm(get_static("Vx")), "xy", cols(Tx), "yn", 1.0, N1, "xn");         // N1 = -(UdT - Vx Tx / 2)
    } else {
        contract(paired ? 0.5 : 1.0, pairm(get_static("Vd")), "xy", cols(Ttd), "yn", 1.0, M, "xn");   // M = 2 Wd - UdT + Vd Tt_d
    }
    if (traces) {
        dev::pair_traces(M.p, nc, cz, 1.0, xs_vv_, xs_oo_, no, nv, stream, quad ? N1.p : nullptr, cu);
        xs_oo_tag_.set(t2, 0, 1);
        xs_vv_tag_.set(t2, 0, 1);
    }
    if (fold) {
        // X_ki = f_ki + w S_ki (:215-220), X_ac = f_ac - w S_ac (:206-212), then Dx into both operands as two strided
        // accumulations each: m[(c,k),(b,k)] += wgt X_bc (X broadcast along k) and m[(c,k),(c,j)] -= wgt X_kj (along c)
        TView Xoo = make_view(arena.alloc(o * o), {o, o}), Xvv = make_view(arena.alloc(v * v), {v, v});
        copy(slice(slice(F, 0, 0, o), 1, 0, o), Xoo);
        axpby(w, make_view(xs_oo_, {o, o}), 1.0, Xoo);
        copy(slice(slice(F, 0, o, nn), 1, o, nn), Xvv);
        axpby(-w, make_view(xs_vv_, {v, v}), 1.0, Xvv);
        auto add_Dx = [&](const TView& m, double wgt) {
            const int64_t ld = m.st[0];
            const int64_t dv[3] = {v, v, o}, sv_in[3] = {1, v, 0}, sv_out[3] = {o * ld, o, ld + 1};            // (c, b, k)
            axpby(wgt, make_view(Xvv.p, 3, dv, sv_in), 1.0, make_view(m.p, 3, dv, sv_out));
            const int64_t dn[3] = {v, o, o}, so_in[3] = {0, o, 1}, so_out[3] = {o * ld + o, ld, 1};           // (c, k, j)
            axpby(-wgt, make_view(Xoo.p, 3, dn, so_in), 1.0, make_view(m.p, 3, dn, so_out));
        };
        add_Dx(M, paired ? 0.25 : 0.5);
        add_Dx(N1, 0.5);
        ring_fold_.set(t2, s.ETd_p);
    }
    if (paired) {
        pair_gemm(1.0, Tx.p, Ttd.p, N1.p, M.p, 0.0, ETx.p, ETd.p);                           // Ex_x = -Xc,  D = Tt_d M_h
    } else {
        // all columns on this rank: nothing is exchanged, and since only Ex + Ex^T enters R (residual_assemble) the slab
        // need not be transposed — Ex_x = Tx N1 and Ex_d = Tt_d M / 2 + Ex_x / 2 with the K-contiguous symmetric amplitudes
        // on the left: the same operand layout as the two builds (the LDS-DMA variant with the better L2 reuse: 6.4 GB of
        // fetches per launch against 13.6 GB for the transposed form, profiles/r02/bench_c3_pmc_hbm_traffic.csv)
        contract(1.0, Tx, "mk", N1, "kn", 0.0, ETx, "mn");                                   // Ex_x = -Xc
        contract(0.5, Ttd, "mk", M, "kn", 0.5, ETd, "mn", "", &ETx);                         // Ex_d = D-term - Xc / 2
    }
}

void Engine::residual_slab(const double* f, const double* t2, double* ETd_p, double* ETx_p, double* L, int rank,
                           int world, unsigned flags, const double* t1, double* QK, const double* P) {
    const bool dcd = flags & PYMES_DCD, dressed = flags & PYMES_USE_DRESSED,
               skip_ladder = flags & (PYMES_SKIP_LADDER | PYMES_SLAB_RINGS_ONLY), skip_rings = flags & PYMES_SLAB_LADDERS_ONLY;
    const bool quad = !dcd;
    const int64_t o = no, v = nv, nn = n, ov = o * v;
    if (world < 1 || rank < 0 || rank >= world) throw Error("residual_slab: bad rank/world");
    if (L && !skip_ladder) check_shard_rank("residual_slab", rank, world);
    const double w = quad ? 1.0 : 0.5;
    TView F = make_view(const_cast<double*>(f), {nn, nn});
    if (L && !skip_ladder) slab_ladders(t2, L, rank, world, flags, t1, QK, P);
    if (skip_rings) return;
    ring_fold_.clear();            // whatever this call writes into ETd / ETx, an earlier folded slab is no longer what they hold
    int64_t c0, c1;
    chunk(ov, rank, world, c0, c1);
    const int64_t nc = c1 - c0;
    if (nc <= 0) return;           // a rank without columns never touches (or needs) the dressed ov blocks
    TView Viajb = block(P_iajb, dressed), Viabj = block(P_iabj, dressed);

    ArenaScope scope(arena);
    auto pairm = [&](double* p) { return make_view(p, {ov, ov}); };
    // Ring fold (one rank, all columns, the V.T sums as traces of the builds): X_ac and X_ki are complete before the two
    // applications, and with the sparse pair matrix  Dx[(c,k),(b,j)] = X_bc d_kj - d_cb X_kj
    //     M -> M + Dx / 2,  N1 -> N1 + Dx / 2     (paired form: M_h = M / 2 -> M_h + Dx / 4)
    // the assembly Ex_d + Ex_d^T + Ex_x(ajbi) + Ex_x(biaj) gains exactly X_ac T_cbij + X_bc T_acij - X_ki T_abkj - X_kj T_abik
    // (ccd.py:231-232 after symmetrisation; the unwanted index placements of the two halves cancel, which needs the equal
    // weights).  v^2 o + v o^2 entries per operand instead of two streaming products over (ov)^2 arrays: no X_ki product,
    // no Td, and the finish does not form X_ac T (ring_fold_).  tests/test_ring_fold.py pins the identity.
    const bool traces = !P && nc == ov;      // the small V.T sums as partial traces of the builds (below; one rank only)
    const bool fold = traces && ring_fold_enabled();
    pair_layouts_of(t2, !fold, flags & kSymTail);
    TView Td = pairm(lay_[0]), Tx = pairm(lay_[1]), Ttd = pairm(lay_[2]);
    TView ETd = slice(pairm(ETd_p), 0, c0, c1), ETx = slice(pairm(ETx_p), 0, c0, c1);
    // column slabs (b,j) in [c0,c1) of the static / dressed right-hand factors, straight from the 4-index blocks:
    //   Wd[(c,k),(b,j)] = V_iabj[k,b,c,j],   UdT[(c,k),(b,j)] = V_iajb[k,b,j,c]
    const int64_t b0 = c0 / o, b1 = (c1 + o - 1) / o;
    auto load_cols = [&](double alpha, const TView& blk, const char* spec, const TView& dst) {
        TView src = slice(blk, 1, b0, b1);                       // only the b values the slab touches
        if (b0 * o == c0 && b1 * o == c1) {
            permute(alpha, src, spec, 0.0, make_view(dst.p, {v, o, b1 - b0, o}), "ckbj");
        } else {
            ArenaScope s2(arena);
            TView tmp = make_view(arena.alloc(ov * (b1 - b0) * o), {ov, (b1 - b0) * o});
            permute(alpha, src, spec, 0.0, make_view(tmp.p, {v, o, b1 - b0, o}), "ckbj");
            copy(slice(tmp, 1, c0 - b0 * o, c1 - b0 * o), dst);
        }
    };
    // ---- the o^3 v^3 terms in four products (three for DCSD).  With pair matrices on (a,i) = a*o + i, all symmetric,
    //   Wd[(c,k),(b,j)] = V~_iabj[k,b,c,j],  Ud^T[(c,k),(b,j)] = V~_iajb[k,b,j,c],  Ld = 2 Vd - Vx  (L_ldkc = 2 g_ldkc - g_lckd)
    // the ten ring products of ccd.py:190-191, :199-204, :233-240 are, for V_pqrs = V_qpsr and T_abij = T_baji, exactly
    //   D-term:  Ex_d  = 1/2 Tt_d (2 Wd - Ud^T + 1/2 Ld Tt_d)            (one build, one application)
    //   C-term:  Xc    = Tx (Ud^T - 1/2 Vx Tx),   Ex_d -= 1/2 Xc,   Ex_x = -Xc     (one build, ONE application, used in both
    //            index placements — the (1/2 + P_ij) of the closed-shell CCSD doubles equations in their C / D form)
    // (numerically identical to the reference's sequence to rounding: tests/test_host_round2.py pins the identity and every
    // golden solve pins the result).  DCSD keeps ccd.py:202-204 only: 2 Wd - Ud^T + Vd Tt_d in the D-term, no build in the
    // C-term.  Column slab [c0,c1): both builds are restricted to the rank's columns n, the applications give rows n.
    auto load_rows = [&](double alpha, const TView& blk, const char* spec, const TView& dst) {
        TView src = slice(blk, 1, b0, b1);                       // only the b values the slab touches
        if (b0 * o == c0 && b1 * o == c1) {
            permute(alpha, src, spec, 0.0, make_view(dst.p, {b1 - b0, o, v, o}), "bjck");
        } else {
            ArenaScope s2(arena);
            TView tmp = make_view(arena.alloc((b1 - b0) * o * ov), {(b1 - b0) * o, ov});
            permute(alpha, src, spec, 0.0, make_view(tmp.p, {b1 - b0, o, v, o}), "bjck");
            copy(slice(tmp, 0, c0 - b0 * o, c1 - b0 * o), dst);
        }
    };
    const RingSlab rs{t2, ETd_p, quad, traces, fold, c0, c1, F, Viajb, Viabj, Tx, Ttd, ETd, ETx, load_cols, load_rows};
    if (nc != ov) slab_rings_rows(rs);
    else slab_rings_cols(rs);
    if (!fold) {
        // :232  Ex[a,b,i,j] -= X_ki T[a,b,k,j]  ->  ET[(b,j),(a,i)] -= sum_k Td[(b,j),(a,k)] X_ki   (Td symmetric)
        ArenaScope s2(arena);
        TView Foo = slice(slice(F, 0, 0, o), 1, 0, o);
        TView Xoo = make_view(arena.alloc(o * o), {o, o});
        copy(Foo, Xoo);
        if (P) {                 // the V.T part was summed over the ranks (slab_prepare)
            axpby(1.0, make_view(const_cast<double*>(P), {o, o}), 1.0, Xoo);
        } else if (traces) {
            axpby(w, make_view(xs_oo_, {o, o}), 1.0, Xoo);                                   // :215-220
        } else {
            TView Tp = make_view(arena.alloc(o * o * v * v), {v, v, o, o});
            permute(1.0, make_view(Ttd.p, {v, o, v, o}), "cidl", 0.0, Tp, "cdli");
            contract(w, make_view(get_static("Vk3"), {v, v, o, o}), "cdlk", Tp, "cdli", 1.0, Xoo, "ki");   // :215-220
        }
        TView Trows = make_view(Td.p + c0 * ov, {nc, v, o});
        TView Erows = make_view(ETd.p, {nc, v, o});
        contract(-1.0, Trows, "nak", Xoo, "ki", 1.0, Erows, "nai");
    }
}

// Small replicated intermediates of residual_slab as K-sharded partial sums (one process per GPU; the caller all-reduces):
//   P = [ X'_ki = w sum_{cdl} Tt[c,d,i,l] V[l,k,d,c]  (o x o;  c in the rank's chunk)
//       | Jp, Jm = 2 V_klcd T_cdij pair-packed       (opp x ldp, opp x ldm;  pairs (c,d) in the rank's chunk) ]
int64_t Engine::slab_prepare_ws_doubles() const {
    const PairDims d = pair_dims();
    return static_cast<int64_t>(no) * no + d.opp * d.ldp + d.opp * d.ldm;
}

void Engine::slab_prepare(const double* t2, double* P, int rank, int world, unsigned flags) {
    const bool dcd = flags & PYMES_DCD;
    const PairDims d = pair_dims();
    const int64_t o = no, v = nv, npp = d.npp, npm = d.npm, opp = d.opp, opm = d.opm, ldp = d.ldp, ldm = d.ldm;
    if (world < 1 || rank < 0 || rank >= world) throw Error("slab_prepare: bad rank/world");
    dev::memset_zero(P, sizeof(double) * slab_prepare_ws_doubles(), stream);
    TView T = make_view(const_cast<double*>(t2), {v, v, o, o});
    ArenaScope scope(arena);
    ensure_xs();
    xs_oo_tag_.clear();
    {
        // X'_ki over c in [c0,c1)
        int64_t c0, c1;
        chunk(v, rank, world, c0, c1);
        if (c1 > c0) {
            ArenaScope s2(arena);
            TView Tc = slice(T, 0, c0, c1);                                       // T[c,d,i,l]
            TView Tp = make_view(arena.alloc((c1 - c0) * v * o * o), {c1 - c0, v, o, o});
            permute(2.0, Tc, "cdil", 0.0, Tp, "cdli");                            // Tt[c,d,i,l] = 2 T[c,d,i,l] - T[d,c,i,l]
            permute(-1.0, slice(T, 1, c0, c1), "dcil", 1.0, Tp, "cdli");
            TView Vk3 = slice(make_view(get_static("Vk3"), {v, v, o, o}), 0, c0, c1);
            contract(1.0, Vk3, "cdlk", Tp, "cdli", 0.0, make_view(xs_oo_, {o, o}), "ki");         // :215-220
            axpby(dcd ? 0.5 : 1.0, make_view(xs_oo_, {o, o}), 0.0, make_view(P, {o, o}));
        } else {
            dev::memset_zero(xs_oo_, sizeof(double) * o * o, stream);
        }
        xs_oo_tag_.set(t2, rank, world);       // this rank's partial sum: the singles residual takes ccsd.py:434 from it
    }
    const PackedV Vij = ijab_pack();
    {
        // J over the packed pairs P(c,d) in the rank's chunk (Q(c,d) for the antisymmetric part)
        double* Sp = arena.alloc(npp * ldp);
        double* Am = arena.alloc(std::max<int64_t>(npm * ldm, 1));
        dev::ladder_pack_T(t2, nullptr, Sp, Am, no, nv, dev::PACK_ROW_HALF, ldp, ldm, stream);
        int64_t k0, k1;
        chunk(npp, rank, world, k0, k1);
        if (k1 > k0)
            contract(2.0, slice(packed_rows(Vij.Vp, opp, npp), 1, k0, k1), "rk",
                     slice(pitched(Sp, npp, opp, ldp), 0, k0, k1), "kn", 0.0, pitched(P + o * o, opp, opp, ldp), "rn");
        chunk(npm, rank, world, k0, k1);
        if (opm > 0 && k1 > k0)
            contract(2.0, slice(packed_rows(Vij.Vm, opp, npm), 1, k0, k1), "rk",
                     slice(pitched(Am, npm, opm, ldm), 0, k0, k1), "kn", 0.0, pitched(P + o * o + opp * ldp, opp, opm, ldm), "rn");
    }
}

void Engine::residual_finish(const double* f, const double* t2, const double* ETd_p, const double* ETx_p,
                             const double* L, double* r2, unsigned flags, const double* t1, const double* QK) {
    const bool dcd = flags & PYMES_DCD, dressed = flags & PYMES_USE_DRESSED, skip_ladder = flags & PYMES_SKIP_LADDER;
    const bool quad = !dcd;
    const int64_t o = no, v = nv, nn = n;
    const double w = quad ? 1.0 : 0.5;
    TView T = make_view(const_cast<double*>(t2), {v, v, o, o});
    TView R = make_view(r2, {v, v, o, o});
    TView F = make_view(const_cast<double*>(f), {nn, nn});
    TView Fvv = slice(slice(F, 0, o, nn), 1, o, nn);
    TView Vijab = block(P_ijab);
    ArenaScope scope(arena);
    const bool packed = L && !skip_ladder;
    const bool fused = dev::fused_pair_kernels_ok(no);
    // amplitude-side mode: V_abij is read UNDRESSED; its (reduced) T1 dressing Z + Z^T(baji) rides in Exn, see below
    const bool amp_side = t1 && packed;
    const TView Vabij_src = block(P_abij, amp_side ? false : dressed);
    if (!fused) copy(Vabij_src, R);                                                         // :185
    if (!packed) {
        ArenaScope s2(arena);
        if (fused) copy(block(P_abij, dressed), R);
        TView hole = make_view(arena.alloc(o * o * o * o), {o, o, o, o});
        copy(block(P_klij, dressed), hole);                                                 // :178
        if (quad) contract(1.0, Vijab, "klcd", T, "cdij", 1.0, hole, "klij");                // :180
        contract(1.0, hole, "klij", T, "abkl", 1.0, R, "abij");                             // :186
        if (!skip_ladder) contract(1.0, block(P_abcd, dressed), "abcd", T, "cdij", 1.0, R, "abij");   // :187
    } else if (!fused) {
        ladder_sym_unpack(L, r2, 1.0);                  // particle (:187) + hole (:175-186) ladders, pair-packed
    }
    // X_ac = f_ac - w sum Tt[a,d,k,l] V[l,k,d,c]  (:206-221);  Ex += X_ac T[c,b,i,j]  (:231)
    const bool reuse = (flags & PYMES_REUSE_LAYOUTS) && lay_t2_ == t2 && lay_[2];     // Tt_d of the preceding residual_slab on this t2
    const bool have_sum = (flags & PYMES_REUSE_LAYOUTS) && xs_vv_tag_.is(t2, 0, 1);   // ... and its S_ac (all columns on this rank)
    // ... unless the ring operands of the slab of this t2 carried X_ac already (residual_slab, ring fold): Exn then holds
    // only the amplitude-side dressing, or nothing
    const bool folded = ring_fold_.is(t2, ETd_p);
    TView Exn;
    if (!folded) {
        TView Xvv = make_view(arena.alloc(v * v), {v, v});
        copy(Fvv, Xvv);
        if (have_sum) {
            axpby(-w, make_view(xs_vv_, {v, v}), 1.0, Xvv);
            Exn = make_view(arena.alloc(o * o * v * v), {v, v, o, o});
        } else {
            TView Ttd = make_view(reuse ? lay_[2] : arena.alloc(o * o * v * v), {v, o, v, o});
            if (!reuse) {
                permute(2.0, T, "abij", 0.0, Ttd, "aibj");
                permute(-1.0, T, "baij", 1.0, Ttd, "aibj");
            }
            contract(-w, Ttd, "akdl", make_view(get_static("Vk"), {o, v, o, v}), "kdlc", 1.0, Xvv, "ac");
            // a private Tt_d is dead after X_ac and lends its storage to Exn; the kept one must survive
            Exn = make_view(reuse ? arena.alloc(o * o * v * v) : Ttd.p, {v, v, o, o});
        }
        contract(1.0, Xvv, "ac", T, "cbij", 0.0, Exn, "abij");
    }
    xs_oo_tag_.clear();                                               // last reader of the iteration
    xs_vv_tag_.clear();
    if (amp_side) {
        if (!QK) throw Error("residual_finish: QK buffer missing");
        if (folded) Exn = make_view(arena.alloc(o * o * v * v), {v, v, o, o});
        amplitude_side_abij(t1, QK, Exn, 0, nv, nv, false, folded ? 0.0 : 1.0);     // (folded: its first product opens Exn)
    }
    if (fused) {
        if (!Exn.p) {                                                 // folded and nothing dressed: the assembly reads zeros
            Exn = make_view(arena.alloc(o * o * v * v), {v, v, o, o});
            zero(Exn);
        }
        // R = V~_abij (or what R holds already) + ladders + Ex + Ex^T in one pass              (:185-187, :249-252)
        dev::residual_assemble(packed ? Vabij_src.p : r2, packed ? L : nullptr, Exn.p, ETd_p, ETx_p, r2, no,
                               nv, stream, ring_xd_);
        stats.permute_calls++;
        stats.permute_bytes += 8.0 * 5.5 * double(o * o * v * v);
        return;
    }
    if (Exn.p) {
        permute(1.0, Exn, "abij", 1.0, R, "abij");
        permute(1.0, Exn, "baji", 1.0, R, "abij");
    }
    TView ETd = make_view(const_cast<double*>(ETd_p), {v, o, v, o}), ETx = make_view(const_cast<double*>(ETx_p), {v, o, v, o});
    permute(1.0, ETd, "aibj", 1.0, R, "abij");                                              // Ex + Ex^T (:249-252)
    permute(1.0, ETd, "bjai", 1.0, R, "abij");
    permute(1.0, ETx, "ajbi", 1.0, R, "abij");
    permute(1.0, ETx, "biaj", 1.0, R, "abij");
    if (ring_xd_ != 0.0) {                                                                  // Ex_d = D + Ex_x / 2 (residual_slab)
        permute(ring_xd_, ETx, "aibj", 1.0, R, "abij");
        permute(ring_xd_, ETx, "bjai", 1.0, R, "abij");
    }
}

// hf.py:14-18 from the packed blocks: f = h + 2 V_piqi - V_piiq (i occupied)
void Engine::hf_fock_matrix(const double* h_host, double* f_host) {
    const double* dir[4];
    const double* exc[4];
    for (int tp = 0; tp < 2; ++tp)
        for (int tq = 0; tq < 2; ++tq) {
            dir[tp * 2 + tq] = block((tp << 3) | (tq << 1)).p;          // (tp, occ, tq, occ)
            exc[tp * 2 + tq] = block((tp << 3) | tq).p;                 // (tp, occ, occ, tq)
        }
    ArenaScope scope(arena);
    const int64_t nn = n;
    double* h = arena.alloc(nn * nn);
    double* f = arena.alloc(nn * nn);
    dev::memcpy_h2d(h, h_host, sizeof(double) * nn * nn, stream);
    dev::hf_fock(dir, exc, h, f, no, nv, stream);
    dev::memcpy_d2h(f_host, f, sizeof(double) * nn * nn, stream);
}

// The part of the T1 dressing of the residual that is linear in the rows a of R and enters through Ex + Ex^T(baji)
// (amplitude-side mode; exchange symmetry V_pqrs = V_qpsr).  With W_kbij = V_kbij + V_kbcj t_ci + V_kbid t_dj:
//     N[a,b,i,j] += V_abcj t_ci - t_ak (Q_kbij + W_kbij)          for a in [a0,a1)   (+ the (b,a,j,i) halves if asked)
// QK holds Q + W (ladder_t1 forms both for the (k,b) rows of a rank; all-gathered by the caller).  Q_kb carries
// the (c,d)-ket part of the bras (k,b)/(a,l); W the rest of those bras; V_abcj t_ci and its
// partner V_abid t_dj = (V_abcj t_ci)_baji are the (c,j)/(i,d) kets of the bra (a,b).  Together with the undressed
// V_abij in the assembly and the (k,l) bra inside the hole ladder this is all of V~_abij (ccsd.py:322-343).
void Engine::amplitude_side_abij(const double* t1, const double* QK, const TView& N, int64_t a0, int64_t a1,
                                 int64_t b1, bool with_partner, double beta) {
    // N is [a1 - a0][b1][o][o]: rows a in [a0,a1), columns b in [0,b1)
    const int64_t o = no, v = nv;
    TView t = make_view(const_cast<double*>(t1), {v, o});
    TView Qf = make_view(const_cast<double*>(QK), {o, v, o, o});        // Q + W, rows (k,b) plain [i][j] (ladder_t1)
    contract(-1.0, slice(t, 0, a0, a1), "ak", slice(Qf, 1, 0, b1), "kbij", beta, N, "abij");
    if (!with_partner) {
        // N is symmetrised by the caller (N_abij + N_baji, residual_assemble): instead of V_abcj t_ci, whose result has the
        // contracted operand's index in the middle (a transposed temporary and an accumulating permutation, 2.4 GB per
        // iteration at (50,200)), add its partner (V_bacj t_ci)_(ab)(ij swapped) = V_abic t_cj  (V_pqrs = V_qpsr), which
        // the GEMM writes in place
        contract(1.0, slice(slice(block(P_abic), 0, a0, a1), 1, 0, b1), "abic", t, "cj", 1.0, N, "abij");
        return;
    }
    contract(1.0, slice(slice(block(P_abci), 0, a0, a1), 1, 0, b1), "abcj", t, "ci", 1.0, N, "abij");
    // the (b,a,j,i) halves for the same rows a (pair-sharded tail): -t_bk (Q+W)[k,a,j,i] and
    // (V_bacᵢ t_cj =) V_abic t_cj, the latter straight from the block with the roles of the kets exchanged
    contract(-1.0, slice(t, 0, 0, b1), "bk", slice(Qf, 1, a0, a1), "kaji", 1.0, N, "abij");
    contract(1.0, slice(slice(block(P_abic), 0, a0, a1), 1, 0, b1), "abic", t, "cj", 1.0, N, "abij");
}

void Engine::pair_chunk(int rank, int world, int64_t& r0, int64_t& r1) const {
    if (world < 1 || rank < 0 || rank >= world) throw Error("pair_chunk: bad rank/world");
    chunk(pair_dims().npp, rank, world, r0, r1);
}

static int a_of_pair_row(int64_t r) {
    int64_t a = static_cast<int64_t>((std::sqrt(8.0 * static_cast<double>(r) + 1.0) - 1.0) * 0.5);
    while (a * (a + 1) / 2 > r) --a;
    while ((a + 1) * (a + 2) / 2 <= r) ++a;
    return static_cast<int>(a);
}

// The replicated remainder of residual_finish reduced to what the pairs of one rank need: X_ac (v x v, cheap) is
// still formed by everyone; the X_ac.T / t.Q_kb combination N'_ab = N_ab + N_ba^T only for the rows a of the rank's
// pairs; the assembly only for its pairs.  Needs the fused assembly kernel (o x o tile in LDS).
void Engine::residual_finish_pairs(const double* f, const double* t2, const double* ETd_p, const double* ETx_p,
                                   const double* L, double* Rc, unsigned flags, const double* t1, const double* QK,
                                   int rank, int world, const double* Xvv_in) {
    const bool dcd = flags & PYMES_DCD, dressed = flags & PYMES_USE_DRESSED;
    const int64_t o = no, v = nv, nn = n;
    const double w = dcd ? 0.5 : 1.0;
    if (!L) throw Error("residual_finish_pairs: L is required");
    if ((t1 == nullptr) != (QK == nullptr)) throw Error("residual_finish_pairs: t1 and QK must be given together");
    if (!dev::fused_pair_kernels_ok(no)) throw Error("residual_finish_pairs: nocc too large for the fused assembly");
    int64_t r0, r1;
    pair_chunk(rank, world, r0, r1);
    if (r1 <= r0) {
        xs_oo_tag_.clear();
        xs_vv_tag_.clear();
        return;
    }
    const int a0 = a_of_pair_row(r0), a1 = a_of_pair_row(r1 - 1) + 1;
    const int64_t na = a1 - a0;
    TView T = make_view(const_cast<double*>(t2), {v, v, o, o});
    TView F = make_view(const_cast<double*>(f), {nn, nn});
    TView Fvv = slice(slice(F, 0, o, nn), 1, o, nn);
    ArenaScope scope(arena);
    // a one-rank slab without P whose ring operands carried X_ac already (residual_slab, ring fold): no X_ac, no X_ac T
    const bool folded = ring_fold_.is(t2, ETd_p);
    // X_ac = f_ac - w sum Tt[a,d,k,l] V[l,k,d,c]  (ccd.py:206-221): given (all-reduced xvv_partial) or formed here
    TView Xvv = Xvv_in ? make_view(const_cast<double*>(Xvv_in), {v, v}) : make_view(arena.alloc(v * v), {v, v});
    if (!Xvv_in && !folded) {
        ArenaScope s2(arena);
        TView Ttd = make_view(arena.alloc(o * o * v * v), {v, o, v, o});
        permute(2.0, T, "abij", 0.0, Ttd, "aibj");
        permute(-1.0, T, "baij", 1.0, Ttd, "aibj");
        copy(Fvv, Xvv);
        contract(-w, Ttd, "akdl", make_view(get_static("Vk"), {o, v, o, v}), "kdlc", 1.0, Xvv, "ac");
    }
    // N'[a,b,i,j] = X_ac T[c,b,i,j] + X_bc T[c,a,j,i] - t_ak Q[k,b,i,j] - t_bk Q[k,a,j,i]   for a in [a0,a1)   (:231)
    // N'[a,b,i,j] = N[a,b,i,j] + N[b,a,j,i] for a in [a0,a1), N = X_ac T[c,b,i,j] + amplitude_side_abij:
    // the (b,a,j,i) halves are written out term by term (they need row b of X / t and row a of the big operands)
    // only the columns b < a1 are needed (b <= a for every pair of the rank): [na][a1] tiles instead of [na][v]
    const int64_t nb = a1;
    TView Np = make_view(arena.alloc(na * nb * o * o), {na, nb, o, o});
    if (folded) {
        zero(Np);
    } else {
        contract(1.0, slice(Xvv, 0, a0, a1), "ac", slice(T, 1, 0, nb), "cbij", 0.0, Np, "abij");
        contract(1.0, slice(Xvv, 0, 0, nb), "bc", slice(T, 1, a0, a1), "caji", 1.0, Np, "abij");
    }
    if (t1) amplitude_side_abij(t1, QK, Np, a0, a1, nb, true);
    // V_abij is read undressed in the amplitude-side mode (CCSD); CCD/DCD have nothing to dress
    const TView Vabij = block(P_abij, t1 ? false : dressed);
    dev::residual_assemble_pairs(Vabij.p, L, Np.p, ETd_p, ETx_p, Rc, no, nv, r0, r1, a0, static_cast<int>(nb), stream, ring_xd_);
    stats.permute_calls++;
    stats.permute_bytes += 8.0 * 5.5 * double(r1 - r0) * 2.0 * double(o * o);
    xs_oo_tag_.clear();                                               // last call of the iteration
    xs_vv_tag_.clear();
}

// rows a in [a0,a1) of the T1-dressed V_abcd (ccsd.py:414-419): what a rank needs for its ladder rows.
// lower_only: only the entries with b <= a are produced (all the pair-packed ladder reads), in a-blocks of
// 32 rows with b < block end — 56 % of the traffic of the full rows at nv = 200.
void Engine::dress_abcd_rows(const double* t1, int a0, int a1, bool lower_only) {
    refuse_if_sharded("dress_abcd_rows");
    refuse_if_direct("dress_abcd_rows");
    if (a0 < 0 || a1 > nv || a0 > a1) throw Error("dress_abcd_rows: bad range");
    if (a0 == a1) return;
    TView t = make_view(const_cast<double*>(t1), {(int64_t)nv, (int64_t)no});
    TView full = block_view(ensure_dressed(P_abcd), P_abcd);
    ArenaScope scope(arena);
    TView oth = block_view(arena.alloc(block_size(P_iabc)), P_iabc);
    const TView raw_iabc = block(P_iabc);
    contract(-1.0, t, "qy", block(P_ijab), "xyrs", 1.0, oth, "xqrs", "x", &raw_iabc);                 // dressed iabc (:385-388)
    const int step = lower_only ? 32 : (a1 - a0);
    for (int p0 = a0; p0 < a1; p0 += step) {
        const int p1 = std::min(a1, p0 + step);
        const int64_t qmax = lower_only ? p1 : nv;
        auto cut = [&](const TView& x) { return slice(slice(x, 0, p0, p1), 1, 0, qmax); };
        TView dst = cut(full);
        const TView raw = cut(block(P_abcd));
        // dst[p,q,r,s] = V[p,q,r,s] - sum_x t[q,x] V_aibc[p,x,r,s]                                   (:416, + copy)
        contract(-1.0, slice(t, 0, 0, qmax), "qx", slice(block(P_aibc), 0, p0, p1), "pxrs", 1.0, dst, "pqrs", "p", &raw);
        // dst[p,q,r,s] -= sum_x t[p,x] V~_iabc[x,q,r,s]                                              (:415, :417)
        contract(-1.0, slice(t, 0, p0, p1), "px", slice(oth, 1, 0, qmax), "xqrs", 1.0, dst, "pqrs");
    }
    if (lpack_.dressed) lpack_.valid = false;
}

void Engine::ladder(const double* t2, double* r2, int a0, int a1, bool dressed, double beta) {
    refuse_if_sharded("ladder");
    refuse_if_direct("ladder");
    const int64_t o = no, v = nv;
    if (a0 < 0 || a1 > nv || a0 > a1) throw Error("ladder: bad a-range");
    if (a0 == a1) return;
    TView T = make_view(const_cast<double*>(t2), {v, v, o, o});
    TView R = slice(make_view(r2, {v, v, o, o}), 0, a0, a1);
    TView Vs = slice(block(P_abcd, dressed), 0, a0, a1);
    contract(1.0, Vs, "abcd", T, "cdij", beta, R, "abij");                                   // ccd.py:187
}

bool Engine::ensure_ladder_pack(int64_t row0, int64_t row1, bool dressed) {
    if (lpack_.valid && lpack_.dressed == dressed && lpack_.row0 == row0 && lpack_.row1 == row1) return false;
    const PairDims d = pair_dims();
    const int64_t rows = row1 - row0;
    if (!lpack_.Vp || lpack_.row1 - lpack_.row0 != rows) {
        dev::stream_sync(stream);
        dev::dfree(lpack_.Vp);
        dev::dfree(lpack_.Vm);
        lpack_.Vp = lpack_.Vm = nullptr;
        lpack_.Vp = static_cast<double*>(dev::dmalloc(sizeof(double) * rows * d.vlp));
        lpack_.Vm = static_cast<double*>(dev::dmalloc(sizeof(double) * rows * d.vlm));
    }
    dev::ladder_pack_V(block(P_abcd, dressed).p, lpack_.Vp, lpack_.Vm, nv, nv, row0, row1, stream, d.vlp, d.vlm);
    lpack_.row0 = row0; lpack_.row1 = row1; lpack_.dressed = dressed; lpack_.valid = true;
    return true;
}

Engine::PackedV Engine::ladder_rows(const char* who, int64_t row0, int64_t row1, bool dressed) {
    // (factor-direct: the undressed ladders never come here, they build their rows chunk by chunk)
    if (direct_.on) refuse_if_direct(dressed ? (std::string(who) + " with the dressed V_abcd").c_str() : who);
    if (shard_on_) {
        check_shard_rows(who, row0, row1, dressed);
        return {srows_.Vp, srows_.Vm, false};
    }
    const bool packed = ensure_ladder_pack(row0, row1, dressed);
    return {lpack_.Vp, lpack_.Vm, packed};
}

Engine::PackedV Engine::ijab_pack() {
    const bool packed = !static_.count("VpIjab");
    if (packed) {
        const PairDims d = pair_dims();
        double* vp = new_static("VpIjab", d.opp * d.vlp);
        double* vm = new_static("VmIjab", d.opp * d.vlm);
        dev::ladder_pack_V(block(P_ijab).p, vp, vm, no, nv, 0, d.opp, stream, d.vlp, d.vlm);
    }
    return {static_["VpIjab"], static_["VmIjab"], packed};
}

// Pair-packed ladder.  With V_abcd = V_badc (electron exchange) and T_cdij = T_dcji:
//   L_abij = LS_(ab)(ij) + sgn(a-b) sgn(i-j) LA_(ab)(ij),
//   LS = sum_{c>=d} (V_abcd + V_abdc) f_cd (T_cdij + T_dcij)/2,   LA = sum_{c>d} (V_abcd - V_abdc) (T_cdij - T_dcij)/2
// for a >= b, i >= j only: two GEMMs of v(v+1)/2 x v(v+-1)/2 x o(o+-1)/2 = 1/4 of the flops of ccd.py:187.
void Engine::ladder_sym(const double* t2, double* L, int64_t row0, int64_t row1, bool dressed, int hole) {
    const PairDims d = pair_dims();
    const int64_t o = no, v = nv, npp = d.npp, npm = d.npm, opp = d.opp, opm = d.opm, ldp = d.ldp, ldm = d.ldm;
    if (row0 < 0 || row1 > npp || row0 > row1) throw Error("ladder_sym: bad pair-row range");
    if (hole < 0 || hole > 2) throw Error("ladder_sym: hole must be 0, 1 (CCSD) or 2 (DCSD)");
    if (row0 == row1) return;
    const int64_t rows = row1 - row0;
    const bool direct = direct_.on && !dressed;
    const PackedV V = direct ? PackedV{nullptr, nullptr, false} : ladder_rows("ladder_sym", row0, row1, dressed);
    if (V.packed) {
        stats.permute_calls++;
        stats.permute_bytes += 8.0 * 2.0 * double(rows) * double(v * v);
    }
    ArenaScope scope(arena);
    double* Sp = arena.alloc(npp * ldp);
    double* Am = arena.alloc(std::max<int64_t>(npm * ldm, 1));
    dev::ladder_pack_T(t2, nullptr, Sp, Am, no, nv, dev::PACK_ROW_HALF, ldp, ldm, stream);
    stats.permute_calls++;
    stats.permute_bytes += 8.0 * 2.0 * double(v * v * o * o);
    // L rows [row0,row1): [ LS (opp) | LA (opm) ], row length o*o
    TView Lrows = make_view(L + row0 * o * o, {rows, o * o});
    TView LS = slice(Lrows, 1, 0, opp), LA = slice(Lrows, 1, opp, o * o);
    if (direct) {
        direct_ladder_products(row0, row1, pitched(Sp, npp, opp, ldp), pitched(Am, npm, opm, ldm), LS, LA);
        if (opm > 0 && npm <= 0) zero(LA);
    } else {
        contract(1.0, packed_rows(V.Vp, rows, npp), "rk", pitched(Sp, npp, opp, ldp), "kn", 0.0, LS, "rn");
        if (opm > 0) {
            if (npm > 0) contract(1.0, packed_rows(V.Vm, rows, npm), "rk", pitched(Am, npm, opm, ldm), "kn", 0.0, LA, "rn");
            else zero(LA);
        }
    }
    if (!hole) return;
    // the hole ladder (ccd.py:175-186) in the same rows: I = V~_klij (+ sum_cd V_klcd T_cdij for CCSD, from the halves of T
    // packed above)
    hole_ladder_rows(t2, block(P_klij, dressed).p, L, row0, row1, nullptr, hole == 1 ? Sp : nullptr, hole == 1 ? Am : nullptr);
    stats.permute_calls += 2;
    stats.permute_bytes += 8.0 * 2.0 * double(v * v * o * o);
}

// The particle ladder (ladder_sym without the hole part) for k vectors in ONE batched launch per half: the packed
// integrals V^+- are the shared left operand (batch stride 0), the packed amplitudes of vector z the right operand of
// batch z.  EOM-CCSD builds sigma for every vector of the Davidson subspace per pass (eom_ccsd.py:95-101): at (30,120) one
// vector is 228 tiles on 256 CUs, k vectors are k x 228 tiles with a k-split tail.
void Engine::ladder_sym_multi(const double* const* xs, int k, double* L_all, bool dressed) {
    refuse_if_sharded("ladder_sym_multi");
    refuse_if_direct("ladder_sym_multi");
    const PairDims d = pair_dims();
    const int64_t o = no, v = nv, npp = d.npp, npm = d.npm, opp = d.opp, opm = d.opm, ldp = d.ldp, ldm = d.ldm;
    if (k < 1) return;
    if (ensure_ladder_pack(0, npp, dressed)) {
        stats.permute_calls++;
        stats.permute_bytes += 8.0 * 2.0 * double(npp) * double(v * v);
    }
    ArenaScope scope(arena);
    const int64_t sp_sz = npp * ldp, am_sz = std::max<int64_t>(npm * ldm, 2);
    double* Sp = arena.alloc(k * sp_sz);
    double* Am = arena.alloc(k * am_sz);
    for (int z = 0; z < k; ++z)
        dev::ladder_pack_T(xs[z], nullptr, Sp + z * sp_sz, Am + z * am_sz, no, nv, dev::PACK_ROW_HALF, ldp, ldm, stream);
    stats.permute_calls += k;
    stats.permute_bytes += 8.0 * 2.0 * double(k) * double(v * v * o * o);
    // operands with explicit batch strides: B_z = Sp + z sp_sz ([npp][ldp], columns 0..opp), C_z = L_all + z npp o^2
    int64_t bd[3] = {k, npp, opp}, bs[3] = {sp_sz, ldp, 1}, cd[3] = {k, npp, opp}, cs[3] = {npp * o * o, o * o, 1};
    contract(1.0, packed_rows(lpack_.Vp, npp, npp), "rk", make_view(Sp, 3, bd, bs), "zkn", 0.0, make_view(L_all, 3, cd, cs), "zrn", "z");
    if (opm > 0) {
        if (npm > 0) {
            int64_t bd2[3] = {k, npm, opm}, bs2[3] = {am_sz, ldm, 1}, cd2[3] = {k, npp, opm};
            contract(1.0, packed_rows(lpack_.Vm, npp, npm), "rk", make_view(Am, 3, bd2, bs2), "zkn", 0.0,
                     make_view(L_all + opp, 3, cd2, cs), "zrn", "z");
        } else {
            int64_t cd2[3] = {k, npp, opm};
            zero(make_view(L_all + opp, 3, cd2, cs));
        }
    }
}

void Engine::ladder_sym_adjoint_multi(const double* const* xs, int k, double* LSp, double* LAp, bool dressed) {
    refuse_if_sharded("ladder_sym_adjoint_multi");
    refuse_if_direct("ladder_sym_adjoint_multi");
    if (k < 1) return;
    const PairDims d = pair_dims();
    const int64_t o = no, v = nv, npp = d.npp, npm = d.npm, opm = d.opm, ldp = d.adj_ldp, ldm = d.adj_ldm, K = k;
    if (ensure_ladder_pack(0, npp, dressed)) {
        stats.permute_calls++;
        stats.permute_bytes += 8.0 * 2.0 * double(npp) * double(v * v);
    }
    ArenaScope scope(arena);
    // the summed pair (a,b) is the ROW index of V+ / V-: the antisymmetric half of x is packed by the same pairs P(a,b)
    // (PACK_AM_PROWS; the rows of diagonal pairs are zero, as the rows of V- are).  The packed halves of vector z lie in the
    // columns [z ld, (z + 1) ld) of rows of pitch k ld (the pad columns zeroed: they go through the product as columns of their own)
    double* Sp = arena.alloc(npp * K * ldp);
    double* Am = arena.alloc(npp * K * ldm);
    zero(make_view(Sp, {npp * K * ldp}));
    zero(make_view(Am, {npp * K * ldm}));
    for (int z = 0; z < k; ++z)
        dev::ladder_pack_T(xs[z], nullptr, Sp + z * ldp, Am + z * ldm, no, nv, dev::PACK_ROW_HALF | dev::PACK_AM_PROWS, K * ldp,
                           K * ldm, stream);
    stats.permute_calls += k;
    stats.permute_bytes += 8.0 * 2.0 * double(k) * double(v * v * o * o);
    contract(1.0, packed_rows(lpack_.Vp, npp, npp), "kr", make_view(Sp, {npp, K * ldp}), "kn", 0.0, make_view(LSp, {npp, K * ldp}), "rn");
    if (opm > 0 && npm > 0)
        contract(1.0, packed_rows(lpack_.Vm, npp, npm), "kr", make_view(Am, {npp, K * ldm}), "kn", 0.0,
                 make_view(LAp, {npm, K * ldm}), "rn");
}

// ---- the hole-ladder steps.  HL_abij = sum_kl I_klij X_abkl for I_klij = I_lkji, X_abkl = X_balk, in the pair-packed rows:
// with S/A = (X_abkl +- X_bakl)/2
//   HLS[(a>=b),(i>=j)] = sum_{k>=l} g_kl S_abkl (I_klij + I_lkij),  HLA[(a>b),(i>j)] = sum_{k>l} A_abkl (I_klij - I_lkij)
// and, where I carries a V.T part, (I_klij +- I_lkij)/2 = pack(I) + sum_{c>=d} (V_klcd +- V_kldc) (f_cd S | A)_cdij.
void Engine::hole_operand_pack(const double* I, const HoleOperand& h) {
    const PairDims d = pair_dims();
    if (d.ldp > d.opp) {       // the zero pad row of the K range
        dev::memset_zero(h.Ip + d.opp * d.ldp, sizeof(double) * d.ldp, stream);
        dev::memset_zero(h.Im + d.opp * d.ldm, sizeof(double) * d.ldm, stream);
    }
    dev::ladder_pack_T(I, nullptr, h.Ip, h.Im, no, no, dev::PACK_AM_PROWS, d.ldp, d.ldm, stream);
}

Engine::HoleOperand Engine::hole_operand(const double* I) {
    const PairDims d = pair_dims();
    HoleOperand h;
    h.Ip = arena.alloc(d.ldp * d.ldp);
    h.Im = arena.alloc(d.ldp * d.ldm);
    hole_operand_pack(I, h);
    return h;
}

void Engine::hole_operand_add(const HoleOperand& h, const double* Sp, const double* Am, double beta, bool grouped) {
    const PairDims d = pair_dims();
    TView Ipv = pitched(h.Ip, d.opp, d.opp, d.ldp), Imv = pitched(h.Im, d.opp, d.opm, d.ldm);        // the defined part
    if (!Sp) {
        axpby(2.0, Ipv, 0.0, Ipv);
        if (d.opm > 0) axpby(2.0, Imv, 0.0, Imv);
        return;
    }
    // [opp x npp] . [npp x opp] instead of the o^2 x v^2 x o^2 product of ccd.py:180
    const PackedV V = ijab_pack();
    std::optional<GemmGroupScope> grp;
    if (grouped) grp.emplace(stream);
    contract(2.0, packed_rows(V.Vp, d.opp, d.npp), "rk", pitched(const_cast<double*>(Sp), d.npp, d.opp, d.ldp), "kn", beta, Ipv, "rn");
    if (d.opm > 0 && d.npm > 0)
        contract(2.0, packed_rows(V.Vm, d.opp, d.npm), "rk", pitched(const_cast<double*>(Am), d.npm, d.opm, d.ldm), "kn", beta, Imv, "rn");
    if (grp) grp->close();
    if (d.opm > 0 && d.npm <= 0 && beta != 1.0) axpby(beta, Imv, 0.0, Imv);       // nv = 1: no (c,d) pair in the A half
}

void Engine::hole_ladder_rows(const double* x, const double* I, double* L, int64_t row0, int64_t row1, const double* y,
                              const double* ySp, const double* yAm) {
    const PairDims d = pair_dims();
    const int64_t o = no, npp = d.npp, npm = d.npm, opp = d.opp, opm = d.opm, ldp = d.ldp, ldm = d.ldm;
    TView Lrows = make_view(L + row0 * o * o, {row1 - row0, o * o});
    TView LS = slice(Lrows, 1, 0, opp), LA = slice(Lrows, 1, opp, o * o);
    const HoleOperand h = hole_operand(I);
    if (y) {
        ijab_pack();           // (a first use packs V_klcd ahead of y)
        ArenaScope s2(arena);
        double* Sp = arena.alloc(npp * ldp);
        double* Am = arena.alloc(std::max<int64_t>(npm * ldm, 1));
        dev::ladder_pack_T(y, nullptr, Sp, Am, no, nv, dev::PACK_ROW_HALF, ldp, ldm, stream);
        hole_operand_add(h, Sp, Am, 2.0);
    } else {
        hole_operand_add(h, ySp, yAm, 2.0);
    }
    double* SpR = arena.alloc(npp * ldp);
    double* AmR = arena.alloc(npp * ldp);
    dev::ladder_pack_T(x, nullptr, SpR, AmR, no, nv, dev::PACK_COL_HALF | dev::PACK_AM_PROWS | dev::PACK_AM_PCOLS, ldp, ldp, stream,
                       row0, row1);                   // only the rows this call multiplies
    // the (k,l) pair is the GEMM K index: it runs over the padded pitch (zero pad column in the rows of x, zero pad row in I)
    contract(1.0, slice(make_view(SpR, {npp, ldp}), 0, row0, row1), "rk", pitched(h.Ip, ldp, opp, ldp), "kn", 1.0, LS, "rn");
    if (opm > 0) contract(1.0, slice(make_view(AmR, {npp, ldp}), 0, row0, row1), "rk", pitched(h.Im, ldp, opm, ldm), "kn", 1.0, LA, "rn");
}

// A hole-ladder-shaped term sum_kl I_klij X_abkl in the pair-packed rows of L (added to what the rows hold), for
// I_klij = I_lkji and X_abkl = X_balk: the (k,l) part of ladder_sym for a caller-supplied I (EOM-CCSD: eom_ccsd.py:380-382
// — u2 against V_klij + V_klcd T_cdij, T against V_kldc u2_dcij), 1/4 of the flops of the plain v^2 o^4 product.  With y
// (exchange-symmetric, [v,v,o,o]) the term sum_cd V_klcd y_cdij is added to I on the way, pair-packed too.
void Engine::hole_ladder_packed(const double* x, const double* I, double* L, int64_t row0, int64_t row1, const double* y) {
    if (row0 < 0 || row1 > pair_dims().npp || row0 > row1) throw Error("hole_ladder_packed: bad pair-row range");
    if (row0 == row1) return;
    ArenaScope scope(arena);
    hole_ladder_rows(x, I, L, row0, row1, y);
    stats.permute_calls++;
    stats.permute_bytes += 8.0 * 2.0 * double(row1 - row0) * 2.0 * double(static_cast<int64_t>(no) * no);
}

// hole_ladder_packed for k vectors in batched launches: L_z += rows(x_z) . (2 pack(I_z) [+ 2 V_klcd y_z, pair-packed]), all
// rows.  Entries of xs (and of Is) may all be the same pointer — the EOM-CCSD sigma builds call it once with x_z = u2_z
// against the shared V_klij + V_klcd T_cdij (eom_ccsd.py:380, :382) and once with the shared T against I_z = B5_z +
// V_kldc u2_z (:381): the shared side is packed once and enters the batched GEMM with batch stride 0.
void Engine::hole_ladder_packed_multi(const double* const* xs, const double* const* Is, const double* const* ys, int k,
                                      double* L_all) {
    const PairDims d = pair_dims();
    const int64_t o = no, v = nv, npp = d.npp, npm = d.npm, opp = d.opp, opm = d.opm, ldp = d.ldp, ldm = d.ldm;
    if (k < 1) return;
    bool same_x = true, same_I = true;
    for (int z = 1; z < k; ++z) { same_x = same_x && xs[z] == xs[0]; same_I = same_I && Is[z] == Is[0]; }
    if (ys) same_I = false;
    const int kx = same_x ? 1 : k, ki = same_I ? 1 : k;
    ArenaScope scope(arena);
    const int64_t ip_sz = ldp * ldp, im_sz = ldp * ldm;
    double* Ip = arena.alloc(ki * ip_sz);
    double* Im = arena.alloc(ki * im_sz);
    for (int z = 0; z < ki; ++z) hole_operand_pack(Is[z], {Ip + z * ip_sz, Im + z * im_sz});
    int64_t id[3] = {ki, opp, opp}, is_[3] = {ip_sz, ldp, 1}, md[3] = {ki, opp, std::max<int64_t>(opm, 1)}, ms[3] = {im_sz, ldm, 1};
    TView Ipv = make_view(Ip, 3, id, is_), Imv = make_view(Im, 3, md, ms);
    if (ys) {
        const PackedV Vij = ijab_pack();
        ArenaScope s2(arena);
        const int64_t sp_sz = npp * ldp, am_sz = std::max<int64_t>(npm * ldm, 2);
        double* Sp = arena.alloc(k * sp_sz);
        double* Am = arena.alloc(k * am_sz);
        for (int z = 0; z < k; ++z)
            dev::ladder_pack_T(ys[z], nullptr, Sp + z * sp_sz, Am + z * am_sz, no, nv, dev::PACK_ROW_HALF, ldp, ldm, stream);
        stats.permute_calls += k;
        stats.permute_bytes += 8.0 * 2.0 * double(k) * double(v * v * o * o);
        int64_t bd[3] = {k, npp, opp}, bs[3] = {sp_sz, ldp, 1};
        contract(2.0, packed_rows(Vij.Vp, opp, npp), "rk", make_view(Sp, 3, bd, bs), "zkn", 2.0, Ipv, "zrn", "z");
        if (opm > 0 && npm > 0) {
            int64_t bd2[3] = {k, npm, opm}, bs2[3] = {am_sz, ldm, 1};
            contract(2.0, packed_rows(Vij.Vm, opp, npm), "rk", make_view(Am, 3, bd2, bs2), "zkn", 2.0, Imv, "zrn", "z");
        } else if (opm > 0) {
            axpby(2.0, Imv, 0.0, Imv);
        }
    } else {
        axpby(2.0, Ipv, 0.0, Ipv);
        if (opm > 0) axpby(2.0, Imv, 0.0, Imv);
    }
    const int64_t xr_sz = npp * ldp;
    double* SpR = arena.alloc(kx * xr_sz);
    double* AmR = arena.alloc(kx * xr_sz);
    for (int z = 0; z < kx; ++z)
        dev::ladder_pack_T(xs[z], nullptr, SpR + z * xr_sz, AmR + z * xr_sz, no, nv,
                           dev::PACK_COL_HALF | dev::PACK_AM_PROWS | dev::PACK_AM_PCOLS, ldp, ldp, stream, 0, npp);
    stats.permute_calls += kx;
    stats.permute_bytes += 8.0 * 2.0 * double(kx) * double(npp) * 2.0 * double(o * o);
    // L_z[r][n] += sum_k' X_z[r][k'] I_z[k'][n], K over the padded pitch (zero pad column of X, zero pad row of I)
    int64_t xd[3] = {kx, npp, ldp}, xst[3] = {xr_sz, ldp, 1};
    int64_t ikd[3] = {ki, ldp, opp}, ikm[3] = {ki, ldp, std::max<int64_t>(opm, 1)};
    int64_t cd[3] = {k, npp, opp}, cd2[3] = {k, npp, std::max<int64_t>(opm, 1)}, cs[3] = {npp * o * o, o * o, 1};
    auto drop = [](const TView& t) { return t.dim[0] == 1 ? std::string() : std::string("z"); };
    TView XS = make_view(SpR, 3, xd, xst), XA = make_view(AmR, 3, xd, xst);
    TView IKp = make_view(Ip, 3, ikd, is_), IKm = make_view(Im, 3, ikm, ms);
    auto spec = [&](const TView& t, const char* two) { return drop(t) + two; };
    auto squeeze = [&](const TView& t) {
        if (t.dim[0] != 1) return t;
        int64_t d2[2] = {t.dim[1], t.dim[2]}, s2[2] = {t.st[1], t.st[2]};
        return make_view(t.p, 2, d2, s2);
    };
    contract(1.0, squeeze(XS), spec(XS, "rk").c_str(), squeeze(IKp), spec(IKp, "kn").c_str(), 1.0, make_view(L_all, 3, cd, cs), "zrn", "z");
    if (opm > 0)
        contract(1.0, squeeze(XA), spec(XA, "rk").c_str(), squeeze(IKm), spec(IKm, "kn").c_str(), 1.0,
                 make_view(L_all + opp, 3, cd2, cs), "zrn", "z");
}

// T1 dressing of the ladders on the amplitude side.  With X_a^p = delta_ap - t_ak delta_pk the dressed ladder and the
// (c,d)-ket part of V~_abij are  sum_pq X_a^p X_b^q sum_cd V_pqcd tau_cdij,  tau = T + t1 t1 (exchange-symmetric like T):
//   (p,q) = (a,b): the pair-packed ladder with the UNDRESSED V_abcd, packed once per solve          -> L rows
//   (p,q) = (k,b), (a,l): -t_ak Q_kbij - t_bl Q_laji,  Q_kbij = sum_cd V_kbcd tau_cdij (cd pair-packed) -> QK rows
//   (p,q) = (k,l): t_ak t_bl (V~_klij + V_klcd T_cdij), i.e. the hole ladder (ccd.py:175-186) taken with tau_abkl
//                  instead of T_abkl also covers the (k,l)-bra part of V~_abij                      -> L rows
// V~_abij must therefore be dressed in its reduced form (dress_V bit 16), V~_klij in full; V_abcd is never dressed:
// no o v^4 work and no second copy of V_abcd per iteration.
// Does the bra dressing of the packed V_abcd beat the Q_kb products?  The answer must be the same on every rank (a rank
// that dresses its rows expects QK without Q from all the others), so the model looks at the whole problem — both
// costs shrink with the number of ranks alike: the dressing streams V in and W out (16 B per element) at ~4 TB/s
// effective; the Q products run 2 ov (npp opp + npm opm) flops at ~70 TFLOP/s.  PYMES_LADDER_DRESS=0/1 overrides it.
bool Engine::bra_dress_pays() const {
    const PairDims d = pair_dims();
    const int64_t o = no, v = nv, npp = d.npp, npm = d.npm, opp = d.opp, opm = d.opm;
    if (direct_.on) {
        // factor-direct: there are no stored rows to dress; the T1 dressing rides on tau and the Q_kb products
        if (const char* e = getenv("PYMES_LADDER_DRESS"))
            if (atoi(e) != 0) refuse_if_direct("PYMES_LADDER_DRESS=1 (the bra dressing of the stored rows)");
        return false;
    }
    if (!dev::ladder_dress_ok(no, nv) || dress_off_) return false;
    if (const char* e = getenv("PYMES_LADDER_DRESS")) return atoi(e) != 0;
    const double t_dress = 16.0 * double(npp) * double(npp + npm) / 4.0e12 + 20e-6;
    const double t_q = 2.0 * double(o * v) * (double(npp) * double(opp) + double(npm) * double(opm)) / 70e12;
    return t_dress < 0.8 * t_q;
}

void Engine::ladder_t1(const double* t1, const double* t2, double* L, int64_t row0, int64_t row1, double* QK,
                       int64_t q0, int64_t q1, bool dcd, const double* J) {
    const PairDims d = pair_dims();
    const int64_t o = no, v = nv, ov = o * v, npp = d.npp, npm = d.npm, opp = d.opp, opm = d.opm, ldp = d.ldp, ldm = d.ldm;
    if (row0 < 0 || row1 > npp || row0 > row1) throw Error("ladder_t1: bad pair-row range");
    if (q0 < 0 || q1 > ov || q0 > q1) throw Error("ladder_t1: bad (k,b) row range");
    const int64_t rows = row1 - row0, qrows = q1 - q0;
    // ---- static packs (once per solve) ---------------------------------------------------------
    // (integral sharding: the stored rows take the place of the pack; the dressing writes to its own copy as ever)
    // (factor-direct: no rows are held; they are built chunk by chunk where the product is taken, below)
    const bool direct = direct_.on;
    const PackedV V = rows > 0 && !direct ? ladder_rows("ladder_t1", row0, row1, false) : PackedV{nullptr, nullptr, false};
    // Bra dressing of the rank's rows of the packed V_abcd instead of its share of the Q_kb products: the two rank-no updates of
    // dev::ladder_dress move 2 x 6.5 GB at (50,200) where Q_kbij = sum_cd V_kbcd tau_cdij costs 1.0e12 flops (13.9 ms);
    // the dressed copy W takes the place of V in the ladder product and QK carries the small brackets only.
    bool dress = bra_dress_pays();
    const std::string kkey = ":" + std::to_string(q0) + ":" + std::to_string(q1);
    const std::string rkey = ":" + std::to_string(row0) + ":" + std::to_string(row1);
    if (dress && rows > 0 && (!static_.count("VpKx") || !static_.count("VpDress" + rkey))) {
        // rows (x,k) of V_kxcd (x slow), pair-packed over (c,d): packed in the order of the block, rows transposed; and the
        // dressed copy W of this rank's rows.  Out of memory (2 x 1.6 GB + 2 x 1.6 GB of scratch + the size of the packed
        // rows at (50,200)): one rank falls back to the Q_kb form; among several ranks the choice must not diverge.
        const int64_t lp = d.vlp, lm = d.vlm;
        const bool need_p = !static_.count("VpKx");
        double *tp = nullptr, *tm = nullptr, *px = nullptr, *mx = nullptr, *wp = nullptr, *wm = nullptr;
        bool ok = true;
        auto grab = [&](double*& p, int64_t n) { if (ok) { p = static_cast<double*>(dev::try_dmalloc(sizeof(double) * n)); ok = p != nullptr; } };
        if (!static_.count("VpDress" + rkey)) { grab(wp, rows * lp); grab(wm, rows * lm); }
        if (need_p) { grab(px, ov * lp); grab(mx, ov * lm); grab(tp, ov * lp); grab(tm, ov * lm); }
        if (!ok) {
            for (double* p : {tp, tm, px, mx, wp, wm}) dev::dfree(p);
            if (!(rows == npp && qrows == ov))
                throw Error("ladder_t1: out of device memory for the dressed copy of the packed V_abcd (PYMES_LADDER_DRESS=0 on every rank selects the Q_kb form)");
            dress_off_ = true;
            dress = false;
        } else {
            if (wp) {
                static_["VpDress" + rkey] = wp; static_["VmDress" + rkey] = wm;
                static_doubles_["VpDress" + rkey] = rows * lp; static_doubles_["VmDress" + rkey] = rows * lm;
            }
            if (need_p) {
                static_["VpKx"] = px;
                static_["VmKx"] = mx;
                static_doubles_["VpKx"] = ov * lp; static_doubles_["VmKx"] = ov * lm;
                dev::ladder_pack_V(block(P_iabc).p, tp, tm, 0, nv, 0, ov, stream, lp, lm);
                permute(1.0, make_view(tp, {o, v, lp}), "kxc", 0.0, make_view(px, {v, o, lp}), "xkc");
                permute(1.0, make_view(tm, {o, v, lm}), "kxc", 0.0, make_view(mx, {v, o, lm}), "xkc");
                dev::stream_sync(stream);
                dev::dfree(tp);
                dev::dfree(tm);
            }
        }
    }
    if (!dress && qrows > 0 && !static_.count("VpK" + kkey)) {
        double* vp = new_static("VpK" + kkey, qrows * d.vlp);
        double* vm = new_static("VmK" + kkey, qrows * d.vlm);
        dev::ladder_pack_V(block(P_iabc).p, vp, vm, 0, nv, q0, q1, stream, d.vlp, d.vlm);          // rows (k,b) of V_kbcd as they are
    }
    ijab_pack();               // (with the other static packs, also where J makes this call do without it)
    ArenaScope scope(arena);
    TView Lrows = make_view(L + row0 * o * o, {rows, o * o});
    TView LS = slice(Lrows, 1, 0, opp), LA = slice(Lrows, 1, opp, o * o);
    {
        // ---- particle ladder and Q_kb from tau ----------------------------------------------
        ArenaScope s2(arena);
        double* Sp = arena.alloc(npp * ldp);
        double* Am = arena.alloc(std::max<int64_t>(npm * ldm, 1));
        dev::ladder_pack_T(t2, t1, Sp, Am, no, nv, dev::PACK_ROW_HALF, ldp, ldm, stream);
        stats.permute_calls++;
        stats.permute_bytes += 8.0 * 2.0 * double(v * v * o * o);
        TView SpT = pitched(Sp, npp, opp, ldp), AmT = pitched(Am, npm, opm, ldm);
        const double* Ap = V.Vp;
        const double* Am_ = V.Vm;
        if (dress && rows > 0) {
            ArenaScope s3(arena);
            double* ws = arena.alloc(dev::ladder_dress_ws_doubles(no, nv));
            dev::ladder_dress(Ap, static_["VpKx"], t1, static_["VpDress" + rkey], no, nv, d.vlp, row0, row1, -1.0, ws, stream);
            if (npm > 0)
                dev::ladder_dress(Am_, static_["VmKx"], t1, static_["VmDress" + rkey], no, nv, d.vlm, row0, row1, 1.0, ws, stream);
            Ap = static_["VpDress" + rkey];
            Am_ = static_["VmDress" + rkey];
        }
        // the two halves of the particle ladder (and of Q_kb below) are independent products: small problems run them as
        // one grouped launch (dev::gemm_group_*), big ones keep their LDS-DMA launches
        TView Qp, QS, QA;
        if (qrows > 0 && !dress) {
            Qp = make_view(arena.alloc(qrows * o * o), {qrows, o * o});
            QS = slice(Qp, 1, 0, opp);
            QA = slice(Qp, 1, opp, o * o);
        }
        {
            GemmGroupScope grp(stream);
            if (rows > 0 && !direct) {
                contract(1.0, packed_rows(const_cast<double*>(Ap), rows, npp), "rk", SpT, "kn", 0.0, LS, "rn");
                if (opm > 0 && npm > 0) contract(1.0, packed_rows(const_cast<double*>(Am_), rows, npm), "rk", AmT, "kn", 0.0, LA, "rn");
            }
            if (qrows > 0 && !dress) {
                contract(1.0, packed_rows(static_["VpK" + kkey], qrows, npp), "rk", SpT, "kn", 0.0, QS, "rn");
                if (opm > 0 && npm > 0) contract(1.0, packed_rows(static_["VmK" + kkey], qrows, npm), "rk", AmT, "kn", 0.0, QA, "rn");
            }
            grp.close();
        }
        if (rows > 0 && direct) direct_ladder_products(row0, row1, SpT, AmT, LS, LA);
        if (rows > 0 && opm > 0 && npm <= 0) zero(LA);
        if (qrows > 0 && dress) {
            // QK = W_kbij alone (ccsd.py:322-343, the (i,j)-, (c,j)- and (i,d)-ket parts of the bras (k,b))
            TView t = make_view(const_cast<double*>(t1), {v, o});
            TView Qr = make_view(QK + q0 * o * o, {qrows, o, o});
            axpby(1.0, make_view(block(P_iajk).p + q0 * o * o, {qrows, o, o}), 0.0, Qr);
            contract(1.0, make_view(block(P_iabj).p + q0 * v * o, {qrows, v, o}), "qcj", t, "ci", 1.0, Qr, "qij", "q");
            contract(1.0, make_view(block(P_iajb).p + q0 * o * v, {qrows, o, v}), "qid", t, "dj", 1.0, Qr, "qij");
        } else if (qrows > 0) {
            // rows (k,b) in [q0,q1) of Q_kbij + W_kbij, plain [i][j]: the pair-packed product [ QS | QA ] is unpacked
            // into the exchange buffer and the small brackets of amplitude_side_abij are added for the same rows, so
            // that they are sharded with Q instead of being repeated by every rank
            if (opm > 0 && npm <= 0) zero(QA);
            dev::rows_unpack(Qp.p, QK + q0 * o * o, qrows, no, stream);
            TView t = make_view(const_cast<double*>(t1), {v, o});
            TView Qr = make_view(QK + q0 * o * o, {qrows, o, o});
            axpby(1.0, make_view(block(P_iajk).p + q0 * o * o, {qrows, o, o}), 1.0, Qr);
            contract(1.0, make_view(block(P_iabj).p + q0 * v * o, {qrows, v, o}), "qcj", t, "ci", 1.0, Qr, "qij", "q");
            contract(1.0, make_view(block(P_iajb).p + q0 * o * v, {qrows, o, v}), "qid", t, "dj", 1.0, Qr, "qij");
        }
    }
    if (rows == 0) return;
    // ---- hole ladder rows.  Ifull = V~_klij + V_klcd T_cdij (pair-packed, doubled as in ladder_sym) ------
    // The (k,l) pair is the GEMM K index here: it runs over the padded pitch ldp (zero pad column in the rows of
    // T / tau, zero pad row in I) so that both operands qualify for 16-byte loads.
    const HoleOperand h = hole_operand(block(P_klij, true).p);
    TView Ipv = pitched(h.Ip, opp, opp, ldp), Imv = pitched(h.Im, opp, opm, ldm);        // the defined part
    TView IpK = pitched(h.Ip, ldp, opp, ldp), ImK = pitched(h.Im, ldp, opm, ldm);        // with the zero pad row
    double* SpR = arena.alloc(npp * ldp);
    double* AmR = arena.alloc(npp * ldp);
    const int rflags = dev::PACK_COL_HALF | dev::PACK_AM_PROWS | dev::PACK_AM_PCOLS;
    auto rowsS = [&]() { return slice(make_view(SpR, {npp, ldp}), 0, row0, row1); };
    auto rowsA = [&]() { return slice(make_view(AmR, {npp, ldp}), 0, row0, row1); };
    if (dcd) {
        // DCSD keeps only V~_klij in the hole ladder proper (ccd.py:178), but the (k,l)-bra part still sees Ifull
        hole_operand_add(h, nullptr, nullptr, 2.0);
        dev::ladder_pack_T(t2, nullptr, SpR, AmR, no, nv, rflags, ldp, ldp, stream, row0, row1);
        contract(1.0, rowsS(), "rk", IpK, "kn", 1.0, LS, "rn");
        if (opm > 0) contract(1.0, rowsA(), "rk", ImK, "kn", 1.0, LA, "rn");
    }
    const double bI = dcd ? 1.0 : 2.0;         // dcd: Ip already holds 2 pack(V~_klij)
    if (J) {       // 2 V_klcd T_cdij (pair-packed) was summed over the ranks (slab_prepare): [ Jp (opp x ldp) | Jm (opp x ldm) ]
        double* j = const_cast<double*>(J);
        axpby(1.0, pitched(j, opp, opp, ldp), bI, Ipv);
        if (opm > 0) axpby(1.0, pitched(j + opp * ldp, opp, opm, ldm), bI, Imv);
    } else {
        ArenaScope s2(arena);
        double* Sp = arena.alloc(npp * ldp);
        double* Am = arena.alloc(std::max<int64_t>(npm * ldm, 1));
        dev::ladder_pack_T(t2, nullptr, Sp, Am, no, nv, dev::PACK_ROW_HALF, ldp, ldm, stream);
        hole_operand_add(h, Sp, Am, bI, true);
    }
    // CCSD: rows of tau against Ifull;  DCSD: rows of t1 t1 against Ifull (rows of T were taken above)
    dev::ladder_pack_T(dcd ? nullptr : t2, t1, SpR, AmR, no, nv, rflags, ldp, ldp, stream, row0, row1);   // this rank's rows
    stats.permute_calls += 3;
    stats.permute_bytes += 8.0 * 4.0 * double(v * v * o * o);
    GemmGroupScope grp(stream);
    contract(1.0, rowsS(), "rk", IpK, "kn", 1.0, LS, "rn");
    if (opm > 0) contract(1.0, rowsA(), "rk", ImK, "kn", 1.0, LA, "rn");
    grp.close();
}

void Engine::ladder_sym_unpack(const double* L, double* r2, double beta) {
    dev::ladder_unpack(L, r2, beta, no, nv, stream);
    stats.permute_calls++;
    stats.permute_bytes += 8.0 * 2.5 * double(nv) * nv * no * no;
}

// -----------------------------------------------------------------------------------
// ccsd.py:226-288   dressed Fock matrix, term by term (grouped; no symmetry assumed)
//   G = 2 G1 - G2,  G1[a,c] = t_bj V_iabc[j,a,b,c],  G2[a,c] = t_bj V_iabc[j,a,c,b]
//   Mm = 2 J1 - J2, J1[k,c] = t_bj V_ijab[j,k,b,c],  J2[k,c] = t_bj V_ijab[j,k,c,b]
//   L = 2 L1 - L2,  L1[k,i] = t_bj V_ijak[j,k,b,i],  L2[k,i] = t_bj V_ijka[j,k,i,b]
//   K1[i,a] = t_bj V_iabj[j,a,b,i],  K2[a,i] = t_bj V_iajb[j,a,i,b]
//   f~_ov = f_ov + 2 K1 - J2                                          (:257-258)
//   f~_oo = f_oo + L + f_ov t + Mm t                                  (:275-279)
//   f~_vv = f_vv + G - t f_ov - t Mm                                  (:282-286)
//   f~_vo = f_vo - t f_oo + f_vv t - t (f_ov t) + 2 K1^T - K2 - t L + G t - t Mm t   (:260-272)
// -----------------------------------------------------------------------------------
// The dressed Fock matrix is built in two stages.  Stage 1: the eight intermediates that contract T1 with a V block over
// (b,j) — linear in V, so a rank may sum over its chunk of the occupied index j only (one process per GPU: the partial
// buffers are all-reduced, 0.7 MB at (50,200)); W = [ G1 (v,v) | G2 (v,v) | J1 (o,v) | J2 (o,v) | L1 (o,o) | L2 (o,o) |
// K1 (o,v) | K2 (v,o) ], every piece written by ONE matrix-vector product (beta = 0): they are independent and go to the
// device as one batched launch (dev::gemv_batch_begin/end).  Stage 2: the combinations G = 2 G1 - G2, ... and their
// products with T1 and f (matrices of n^2 elements) in two small kernels (dev::fock_finish).
int64_t Engine::dress_fock_ws_doubles() const {
    const int64_t o = no, v = nv;
    return 2 * v * v + 4 * o * v + 2 * o * o;
}

void Engine::dress_fock_partial(const double* t1, double* W, int rank, int world) {
    const int64_t o = no, v = nv;
    if (world < 1 || rank < 0 || rank >= world) throw Error("dress_fock_partial: bad rank/world");
    int64_t j0, j1;
    chunk(o, rank, world, j0, j1);
    TView G1 = make_view(W, {v, v}), G2 = make_view(G1.p + v * v, {v, v}), J1 = make_view(G2.p + v * v, {o, v}),
          J2 = make_view(J1.p + o * v, {o, v}), L1 = make_view(J2.p + o * v, {o, o}), L2 = make_view(L1.p + o * o, {o, o}),
          K1 = make_view(L2.p + o * o, {o, v}), K2 = make_view(K1.p + o * v, {v, o});
    if (j1 <= j0) {
        dev::memset_zero(W, sizeof(double) * dress_fock_ws_doubles(), stream);
        return;
    }
    TView t = slice(make_view(const_cast<double*>(t1), {v, o}), 1, j0, j1);
    const bool all = (j0 == 0 && j1 == o);       // whole blocks: the planner may reuse its cached transposed copies
    auto js = [&](int pat) { return all ? block(pat) : slice(block(pat), 0, j0, j1); };
    // the two sums over the o v^3 block in one pass over it as stored (no transposed static copies of the block)
    const bool fused_g12 = dev::fock_g12_ok(nv);
    if (fused_g12) {
        ArenaScope s2(arena);
        const int ja = static_cast<int>(j0), jb = static_cast<int>(j1);
        double* ws = arena.alloc(dev::fock_g12_ws_doubles(nv, nv, jb - ja));
        dev::fock_g12(block(P_iabc).p, t1, G1.p, G2.p, no, nv, nv, ja, jb, ws, stream);
        double* ws2 = arena.alloc(dev::fock_g12_ws_doubles(nv, no, jb - ja));
        dev::fock_g12(block(P_ijab).p, t1, J1.p, J2.p, no, nv, no, ja, jb, ws2, stream);
    }
    struct Batch {
        Batch() { dev::gemv_batch_begin(); }
        ~Batch() { try { dev::gemv_batch_end(); } catch (...) {} }
    };
    {
        Batch batch;
        if (!fused_g12) {
            contract(1.0, t, "bj", js(P_iabc), "jabc", 0.0, G1, "ac");
            contract(1.0, t, "bj", js(P_iabc), "jacb", 0.0, G2, "ac");
        }
        if (!fused_g12) {
            contract(1.0, t, "bj", js(P_ijab), "jkbc", 0.0, J1, "kc");
            contract(1.0, t, "bj", js(P_ijab), "jkcb", 0.0, J2, "kc");
        }
        contract(1.0, t, "bj", js(P_ijak), "jkbi", 0.0, L1, "ki");
        contract(1.0, t, "bj", js(P_ijka), "jkib", 0.0, L2, "ki");
        contract(1.0, t, "bj", js(P_iabj), "jabi", 0.0, K1, "ia");
        contract(1.0, t, "bj", js(P_iajb), "jaib", 0.0, K2, "ai");
        dev::gemv_batch_end();           // (errors surface here; the guard only covers an exception on the way)
    }
}

void Engine::dress_fock_finish(const double* f, const double* t1, const double* W, double* fd) {
    ArenaScope scope(arena);
    dev::fock_finish(f, t1, W, fd, arena.alloc(static_cast<int64_t>(no) * no), no, nv, stream);
}

void Engine::dress_fock(const double* f, const double* t1, double* fd) {
    ArenaScope scope(arena);
    double* W = arena.alloc(dress_fock_ws_doubles());
    dress_fock_partial(t1, W, 0, 1);
    dress_fock_finish(f, t1, W, fd);
}

// X_ac = f_ac - w sum_{kdl} Tt[a,d,k,l] V[l,k,d,c] (ccd.py:206-221), the sum restricted to this rank's chunk of k (one
// process per GPU; f_ac enters on rank 0 only): v x v partial results to be all-reduced
void Engine::xvv_partial(const double* f, const double* t2, double* Xvv_p, int rank, int world, unsigned flags) {
    const bool dcd = flags & PYMES_DCD;
    const int64_t o = no, v = nv, nn = n;
    if (world < 1 || rank < 0 || rank >= world) throw Error("xvv_partial: bad rank/world");
    int64_t k0, k1;
    chunk(o, rank, world, k0, k1);
    TView Xvv = make_view(Xvv_p, {v, v});
    TView F = make_view(const_cast<double*>(f), {nn, nn});
    if (rank == 0) copy(slice(slice(F, 0, o, nn), 1, o, nn), Xvv);
    else zero(Xvv);
    ensure_xs();
    xs_vv_tag_.clear();
    TView S = make_view(xs_vv_, {v, v});
    if (k1 <= k0) {
        zero(S);
    } else {
        ArenaScope scope(arena);
        TView T = make_view(const_cast<double*>(t2), {v, v, o, o});
        TView Tk = slice(T, 2, k0, k1);                                      // T[a,d,k,l], k in the chunk
        TView Ttd = make_view(arena.alloc(v * (k1 - k0) * v * o), {v, k1 - k0, v, o});
        permute(2.0, Tk, "adkl", 0.0, Ttd, "akdl");
        permute(-1.0, Tk, "dakl", 1.0, Ttd, "akdl");
        TView Vk = slice(make_view(get_static("Vk"), {o, v, o, v}), 0, k0, k1);
        contract(1.0, Ttd, "akdl", Vk, "kdlc", 0.0, S, "ac");
        axpby(dcd ? -0.5 : -1.0, S, 1.0, Xvv);
    }
    xs_vv_tag_.set(t2, rank, world);       // this rank's partial sum: the singles residual takes ccsd.py:436 from it
}

// -----------------------------------------------------------------------------------
// ccsd.py:290-421   exp(-T1) V exp(T1), block by block.
// A bra index that is virtual in the target block picks up  -t[a,k] x (occupied source),
// a ket index that is occupied in the target picks up  +(virtual source) x t[c,i]; sources
// are always undressed blocks (checked term by term by the oracle).
// Implemented as a recursion of one-index transforms: ket indices first (they shrink
// v -> o), bra indices last.
// -----------------------------------------------------------------------------------
// reduced (V_abij only, pos = {3,2,1,0}): leave out the terms with both kets virtual (V_pqcd t_ci t_dj) and the
// terms with both bras occupied (t_ak t_bl V~_klrs); ladder_t1 carries them through tau and the hole ladder.
void Engine::dressed_into(int pattern, const std::vector<int>& pos, int k, const TView& t1v, const TView& dst,
                          bool reduced, const int64_t* cut) {
    // cut = {p0, p1, q0, q1} (or null): only the range [p0,p1) of the first and [q0,q1) of the second index are
    // produced (an empty range = the whole index; a cut index must be virtual in the requested block); dst is already
    // cut.  Every block in which such an index is still that virtual index is read through the same cut; the
    // transform of the index itself (x == 0 / 1) restricts the rows of t1 instead.
    auto has = [&](int axis) { return cut && cut[2 * axis + 1] > cut[2 * axis]; };
    auto cutq = [&](TView v, int pat) {
        for (int axis = 0; axis < 2; ++axis)
            if (has(axis) && (pat >> (3 - axis) & 1)) v = slice(v, axis, cut[2 * axis], cut[2 * axis + 1]);
        return v;
    };
    if (k == 0) {
        copy(cutq(block(pattern), pattern), dst);
        return;
    }
    // same-type part: when it is the raw block the copy is fused into the product below (C = Cin + ...)
    const bool fuse_copy = (k - 1 == 0);
    if (!fuse_copy) dressed_into(pattern, pos, k - 1, t1v, dst, reduced, cut);
    const TView raw = fuse_copy ? cutq(block(pattern), pattern) : TView();
    const TView* cin = fuse_copy ? &raw : nullptr;
    if (cin) {      // the fused copy needs Cin laid out like C: a cut of the full block vs a compact temporary is not
        bool same = true;
        for (int i = 0; i < 4; ++i) same = same && (raw.dim[i] == 1 || raw.st[i] == dst.st[i]);
        if (!same) {
            copy(raw, dst);
            cin = nullptr;
        }
    }
    const int x = pos[k - 1];
    const int other = pattern ^ (1 << (3 - x));
    int depth = k - 1;                       // dressing depth of the other-type part
    if (reduced && k == 4) depth = 2;        // p -> k: no q -> l on top of it
    if (reduced && k == 2) depth = 0;        // r -> c: no s -> d on top of it
    ArenaScope scope(arena);
    TView oth;
    long memo_key = ((long)other << 8) | (long)depth;
    for (int i = 0; i < depth; ++i) memo_key = (memo_key << 3) | (long)(pos[i] + 1);
    if (depth == 0) {
        oth = cutq(block(other), other);
    } else if (!reduced && dress_memo_.count(memo_key)) {
        oth = dress_memo_[memo_key];        // formed once for all the blocks of this dress_V call (see there)
    } else {
        int64_t d[4];
        for (int i = 0; i < 4; ++i) d[i] = (other >> (3 - i) & 1) ? nv : no;
        for (int axis = 0; axis < 2; ++axis)
            if (has(axis) && (other >> (3 - axis) & 1)) d[axis] = cut[2 * axis + 1] - cut[2 * axis];
        oth = make_view(arena.alloc(d[0] * d[1] * d[2] * d[3]), 4, d, nullptr);
        dressed_into(other, pos, depth, t1v, oth, reduced, cut);
    }
    const TView tcut = (x < 2 && has(x)) ? slice(t1v, 0, cut[2 * x], cut[2 * x + 1]) : t1v;
    switch (x) {
        case 3: contract(1.0, oth, "pqrx", t1v, "xs", 1.0, dst, "pqrs", "", cin); break;
        case 2: contract(1.0, oth, "pqxs", t1v, "xr", 1.0, dst, "pqrs", "pq", cin); break;
        case 1: contract(-1.0, tcut, "qx", oth, "pxrs", 1.0, dst, "pqrs", "p", cin); break;
        case 0: contract(-1.0, tcut, "px", oth, "xqrs", 1.0, dst, "pqrs", "", cin); break;
        default: throw Error("bad index position");
    }
}

void Engine::dress_V(const double* t1, uint32_t mask, const int64_t* cut) {
    ++dress_generation_;
    TView t = make_view(const_cast<double*>(t1), {(int64_t)nv, (int64_t)no});
    for (int axis = 0; axis < 2 && cut; ++axis)
        if (cut[2 * axis] < 0 || cut[2 * axis + 1] > nv || cut[2 * axis] > cut[2 * axis + 1]) throw Error("dress_V: bad index range");
    ArenaScope memo_scope(arena);
    struct MemoGuard {
        std::map<long, TView>& m;
        ~MemoGuard() { m.clear(); }
    } memo_guard{dress_memo_};
    dress_memo_.clear();
    if ((mask >> P_klij & 1u) && (mask >> P_iabj & 1u)) {
        // V_klcj + V_klcd t_dj (ccsd.py:346-352) is also the occupied-bra source of V~_iabj (:378-383): the same
        // transform of the same block — one pass over V_ijab (0.8 GB at (50,200)) instead of two.  Both bra indices are
        // occupied, so an index range of the call does not touch it.
        const int pat = P_klij | 2;                                   // (o,o,v,o)
        const std::vector<int> pos = {3};
        int64_t d[4] = {no, no, nv, no};
        TView oth = make_view(arena.alloc(d[0] * d[1] * d[2] * d[3]), 4, d, nullptr);
        dressed_into(pat, pos, 1, t, oth, false, cut);
        dress_memo_[(((long)pat << 8 | 1L) << 3) | 4L] = oth;
    }
    for (int pat = 0; pat < 16; ++pat) {
        if (!(mask >> pat & 1u)) continue;
        TView dst = block_view(ensure_dressed(pat), pat);
        for (int axis = 0; axis < 2 && cut; ++axis) {
            if (cut[2 * axis + 1] <= cut[2 * axis]) continue;
            if (!(pat >> (3 - axis) & 1)) continue;                   // an occupied index has no range: the whole block
            dst = slice(dst, axis, cut[2 * axis], cut[2 * axis + 1]);
        }
        std::vector<int> pos;
        if (!(pat >> 0 & 1)) pos.push_back(3);   // ket s occupied
        if (!(pat >> 1 & 1)) pos.push_back(2);   // ket r occupied
        if (pat >> 2 & 1) pos.push_back(1);      // bra q virtual
        if (pat >> 3 & 1) pos.push_back(0);      // bra p virtual
        dressed_into(pat, pos, static_cast<int>(pos.size()), t, dst, pat == P_abij && (mask >> 16 & 1u), cut);
        if (pat == P_abcd && lpack_.dressed) lpack_.valid = false;
    }
}

// -----------------------------------------------------------------------------------
// ccsd.py:423-438   singles residual (dressed Fock, UNDRESSED V, explicit T1 factors)
// -----------------------------------------------------------------------------------
void Engine::singles_residual(const double* fd, const double* t1, const double* t2, double* r1) {
    const int64_t o = no, v = nv, nn = n;
    TView D = make_view(const_cast<double*>(fd), {nn, nn});
    TView Dov = slice(slice(D, 0, 0, o), 1, o, nn), Dvo = slice(slice(D, 0, o, nn), 1, 0, o);
    TView t = make_view(const_cast<double*>(t1), {v, o});
    TView T = make_view(const_cast<double*>(t2), {v, v, o, o});
    TView R = make_view(r1, {v, o});
    ArenaScope scope(arena);
    // Tt'[a,b,i,j] = 2 T[a,b,i,j] - T[a,b,j,i]   (:430), held as Tq[a,i,b,j] and P1[j,b,c,i] = Tt'[b,c,i,j]
    TView Tq = make_view(arena.alloc(o * o * v * v), {v, o, v, o});
    TView P1 = make_view(arena.alloc(o * o * v * v), {o, v, v, o});
    permute(2.0, T, "abij", 0.0, Tq, "aibj");
    permute(-1.0, T, "abji", 1.0, Tq, "aibj");
    permute(2.0, T, "bcij", 0.0, P1, "jbci");
    permute(-1.0, T, "bcji", 1.0, P1, "jbci");
    copy(Dvo, R);                                                                            // :431
    contract(1.0, Tq, "aibj", Dov, "jb", 1.0, R, "ai");                                      // :432
    contract(1.0, block(P_aibc), "ajbc", P1, "jbci", 1.0, R, "ai");                          // :433
    TView S2 = make_view(arena.alloc(o * o), {o, o});
    contract(1.0, make_view(get_static("Vjbck"), {o, v, v, o}), "jbck", P1, "jbci", 0.0, S2, "ki");
    contract(-1.0, t, "ak", S2, "ki", 1.0, R, "ai");                                         // :434
    contract(-1.0, Tq, "ajbk", block(P_ijka), "jkib", 1.0, R, "ai");                         // :435
    TView S4 = make_view(arena.alloc(v * v), {v, v});
    contract(1.0, Tq, "ajbk", block(P_ijab), "jkcb", 0.0, S4, "ac");
    contract(-1.0, S4, "ac", t, "ci", 1.0, R, "ai");                                         // :436
}

// The same residual as a K-sharded partial sum (one process per GPU; exchange-symmetric T2 only): every term contracts
// over one occupied index j together with virtual ones — (b,j), (j,b,c), (j,b,k) — so rank r sums over its chunk of j and
// the v x o partial results are all-reduced (80 KB at (50,200)); the dressed-Fock term enters on rank 0.  With
// T_abij = T_baji, Tt'[a,b,i,j] = 2 T_abij - T_abji is symmetric as an (a,i) x (b,j) matrix, so one permuted piece
// Tq[a,j,b,k] (j in the chunk) serves ccsd.py:432, :435 and :436; P1[j,b,c,i] = Tt'[b,c,i,j] serves :433 and :434.
void Engine::singles_residual_partial(const double* fd, const double* t1, const double* t2, double* r1, int rank, int world,
                                      bool reuse_layouts) {
    const int64_t o = no, v = nv, nn = n;
    if (world < 1 || rank < 0 || rank >= world) throw Error("singles_residual_partial: bad rank/world");
    int64_t j0, j1;
    chunk(o, rank, world, j0, j1);
    const int64_t nj = j1 - j0;
    TView D = make_view(const_cast<double*>(fd), {nn, nn});
    TView Dov = slice(slice(D, 0, 0, o), 1, o, nn), Dvo = slice(slice(D, 0, o, nn), 1, 0, o);
    TView t = make_view(const_cast<double*>(t1), {v, o});
    TView T = make_view(const_cast<double*>(t2), {v, v, o, o});
    TView R = make_view(r1, {v, o});
    if (rank == 0) copy(Dvo, R);                                                             // :431
    else zero(R);
    // ccsd.py:434 / :436 contract the same sums as X_ki / X_ac (ccd.py:213-220; exchange-symmetric V, T): when the
    // calls before this one have left them (residual_slab with all columns, or slab_prepare / xvv_partial: ANY partition
    // of the sums over the ranks will do, the partial residuals are added up) the two products are not repeated
    const bool have_oo = reuse_layouts && xs_oo_tag_.is(t2, rank, world), have_vv = reuse_layouts && xs_vv_tag_.is(t2, rank, world);
    if (have_oo) contract(-1.0, t, "ak", make_view(xs_oo_, {o, o}), "ki", 1.0, R, "ai");     // :434
    if (have_vv) contract(-1.0, make_view(xs_vv_, {v, v}), "ac", t, "ci", 1.0, R, "ai");     // :436
    if (nj <= 0) return;
    ArenaScope scope(arena);
    TView Tq, P1;
    const char* lp1 = "jbci";
    if (reuse_layouts && lay_t2_ == t2 && lay_[2]) {
        // Tt'[a,b,j,k] = Tt_d[(a,j),(b,k)] (exchange-symmetric T), and Tt_d is a symmetric matrix: both operands are
        // strided views of the layout residual_slab has just built — no transposition at all
        TView Ttd = make_view(lay_[2], {v, o, v, o});
        Tq = slice(Ttd, 1, j0, j1);                                                          // [a, j in chunk, b, k]
        P1 = slice(Ttd, 1, j0, j1);                                                          // read as P1[c,j,b,i]
        lp1 = "cjbi";
    } else {
        Tq = make_view(arena.alloc(v * nj * v * o), {v, nj, v, o});                          // Tq[a,j,b,k], j in the chunk
        P1 = make_view(arena.alloc(nj * v * v * o), {nj, v, v, o});                          // P1[j,b,c,i]
        permute(2.0, slice(T, 2, j0, j1), "abjk", 0.0, Tq, "ajbk");
        permute(-1.0, slice(T, 3, j0, j1), "abkj", 1.0, Tq, "ajbk");
        permute(2.0, slice(T, 3, j0, j1), "bcij", 0.0, P1, "jbci");
        permute(-1.0, slice(T, 2, j0, j1), "bcji", 1.0, P1, "jbci");
    }
    contract(1.0, Tq, "bjai", slice(Dov, 0, j0, j1), "jb", 1.0, R, "ai");                    // :432 (Tt' symmetric)
    // (these products stream 80-MB..3.2-GB blocks into tiny outputs over K = o v^2: each runs alone on the single-buffer
    // streaming kernel, which keeps 4-6 blocks per CU in flight — as ONE grouped launch on the double-buffered group kernel
    // they were slower, 178 against 112 us at (20,80), rocprofv3 round 4)
    contract(1.0, slice(block(P_aibc), 1, j0, j1), "ajbc", P1, lp1, 1.0, R, "ai");           // :433
    if (!have_oo) {
        TView S2 = make_view(arena.alloc(o * o), {o, o});
        contract(1.0, slice(make_view(get_static("Vjbck"), {o, v, v, o}), 0, j0, j1), "jbck", P1, lp1, 0.0, S2, "ki");
        contract(-1.0, t, "ak", S2, "ki", 1.0, R, "ai");                                     // :434
    }
    contract(-1.0, Tq, "ajbk", slice(block(P_ijka), 0, j0, j1), "jkib", 1.0, R, "ai");       // :435
    if (!have_vv) {
        TView S4 = make_view(arena.alloc(v * v), {v, v});
        contract(1.0, Tq, "ajbk", slice(block(P_ijab), 0, j0, j1), "jkcb", 0.0, S4, "ac");
        contract(-1.0, S4, "ac", t, "ci", 1.0, R, "ai");                                     // :436
    }
}

// -----------------------------------------------------------------------------------
// ccsd.py:176-179, ccd.py:123-124
// -----------------------------------------------------------------------------------
void Engine::cc_update(double* t, double* dt, const double* r, double shift, double delta, int rank) {
    if (rank != 2 && rank != 4) throw Error("cc_update: rank must be 2 (T1) or 4 (T2)");
    need_eps("cc_update");
    dev::cc_update(t, dt, r, eps_o, eps_v, shift, delta, no, nv, rank, stream);
}

// -----------------------------------------------------------------------------------
// ccsd.py:458-466 and ccd.py:256-262
// -----------------------------------------------------------------------------------
// ---- whole steps ------------------------------------------------------------------------------------------------------------
void Engine::ccsd_residuals(const double* f, const double* t1, const double* t2, unsigned flags, double* r1, double* r2) {
    refuse_if_sharded("ccsd_residuals (single rank)");
    const int64_t o = no, v = nv, ov = o * v, npp = v * (v + 1) / 2;
    if (!res_ETd_) {
        // all five or none: a failed allocation in the middle must not leave a half-initialised set behind, and a
        // launch graph that is being recorded cannot allocate (hipMalloc may synchronise)
        if (capturing_) throw Error("ccsd_residuals: the staging buffers must exist before a launch graph is recorded (run one eager pass first)");
        double* got[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
        const int64_t want[5] = {(o + v) * (o + v), ov * ov, ov * ov, npp * o * o, ov * o * o};
        try {
            for (int i = 0; i < 5; ++i) got[i] = scratch_get(want[i]);
        } catch (...) {
            for (double* p : got)
                if (p) scratch_put(p);
            throw;
        }
        res_fd_ = got[0]; res_ETd_ = got[1]; res_ETx_ = got[2]; res_L_ = got[3]; res_QK_ = got[4];
    }
    const unsigned dcd = flags & PYMES_DCD;
    const unsigned sym = PYMES_SYM_LADDER | PYMES_SYM_RINGS, tail = flags & kSymTail;
    if (flags & PYMES_T1_ZERO) {
        residual_slab(f, t2, res_ETd_, res_ETx_, res_L_, 0, 1, dcd | sym | tail);                              // :171
        singles_residual_partial(f, t1, t2, r1, 0, 1, true);                                                   // :167
        residual_finish(f, t2, res_ETd_, res_ETx_, res_L_, r2, dcd | sym | PYMES_REUSE_LAYOUTS);
        return;
    }
    dress_fock(f, t1, res_fd_);                                                                                // :163
    // V_abcd is never dressed: its T1 dressing (:165, ccsd.py:414-419) is carried by tau = T2 + T1 T1 inside the ladders,
    // that of V_abij by Q_kb and two small products inside the finish; only V~_klij, V~_iajb, V~_iabj are formed
    dress_V(t1, (1u << pattern_of_name("klij")) | (1u << pattern_of_name("iajb")) | (1u << pattern_of_name("iabj")));
    residual_slab(res_fd_, t2, res_ETd_, res_ETx_, res_L_, 0, 1, dcd | sym | tail | PYMES_USE_DRESSED, t1, res_QK_);  // :171
    singles_residual_partial(res_fd_, t1, t2, r1, 0, 1, true);                                                 // :167
    residual_finish(res_fd_, t2, res_ETd_, res_ETx_, res_L_, r2, dcd | sym | PYMES_USE_DRESSED | PYMES_REUSE_LAYOUTS, t1, res_QK_);
}

void Engine::ccsd_iterate(const double* f, double* t1, double* t2, unsigned flags, double shift, double delta, double* dt1,
                          double* dt2, double out[6]) {
    refuse_if_sharded("ccsd_iterate (single rank)");
    const int64_t o = no, v = nv;
    if (!res_r1_) {
        if (capturing_) throw Error("ccsd_iterate: the staging buffers must exist before a launch graph is recorded");
        double* r1 = scratch_get(v * o);
        try {
            res_r2_ = scratch_get(v * v * o * o);
        } catch (...) {
            scratch_put(r1);
            throw;
        }
        res_r1_ = r1;
    }
    // (the symmetry-reduced residual is this step's precondition already: T2, R2, dT2 are exchange-symmetric)
    ccsd_residuals(f, t1, t2, flags | kSymTail, res_r1_, res_r2_);            // ccsd.py:161-171
    cc_update_to(t1, dt1, t1, res_r1_, shift, delta, 2);                      // :176-179
    cc_update_to(t2, dt2, t2, res_r2_, shift, delta, 4, true);
    energy_norms(f, t1, t2, dt2, out, true);                                  // :189-197
}

// ---- one process per GPU with the host program's collectives (engine.h; include/pymes_amd.h, pymes_collectives) -----------------
void Engine::set_collectives(const Collectives* c) {
    if (t2_in_flight_) {
        // a loop that was abandoned between finish and the next residuals: its last exchange is completed through the table
        // that started it (nobody reads the result) before that table goes
        t2_in_flight_ = false;
        dev::phase_sync();
        if (coll_.wait(coll_.user, t2_ticket_, stream) != 0) throw Error("collective hook: wait failed");
    }
    if (!c) {
        coll_ = Collectives();
        coll_set_ = false;
        return;
    }
    if (!c->allreduce_start || !c->allgather_start || !c->wait) throw Error("set_collectives: allreduce_start, allgather_start and wait are required");
    if (c->world < 1 || c->rank < 0 || c->rank >= c->world) throw Error("set_collectives: need 0 <= rank < world");
    coll_ = *c;
    coll_set_ = true;
}

namespace {
// the calls into the host program: a failure there (non-zero return) becomes an Error of this library
struct Hooks {
    const Engine::Collectives& c;
    void* stream;
    // (nothing of the library's own may still be queued when the host program orders a collective behind the stream)
    int64_t allreduce(double* buf, int64_t n) const {
        dev::gemm_group_sync();
        dev::phase_sync();
        int64_t t = 0;
        if (c.allreduce_start(c.user, buf, n, stream, &t) != 0) throw Error("collective hook: allreduce_start failed");
        return t;
    }
    int64_t allgather(double* buf, int64_t chunk) const {
        dev::gemm_group_sync();
        dev::phase_sync();
        int64_t t = 0;
        if (c.allgather_start(c.user, buf, chunk, stream, &t) != 0) throw Error("collective hook: allgather_start failed");
        return t;
    }
    void wait(int64_t ticket) const {
        dev::phase_sync();
        if (c.wait(c.user, ticket, stream) != 0) throw Error("collective hook: wait failed");
    }
    void mark(const char* phase) const {
        if (c.mark) {
            dev::phase_sync();
            c.mark(c.user, phase);
        }
    }
};
int64_t chunk_of(int64_t n, int world) { int64_t lo, hi; return chunk(n, 0, world, lo, hi); }
}  // namespace

// ---- owner tiles: what rank `to` reads of the rows of a ring-product matrix that rank `from` computed (pymes_amd/dist.py,
// owner_tile_plan: the same rectangles).  Rank q owns the pairs P(a,b), a in [a0,a1); its assembly reads the tiles
// [(a,.),(b,.)] and [(b,.),(a,.)], b <= a: rows [0, a1 o) x columns [a0 o, a1 o) and rows [a0 o, a1 o) x columns [0, a0 o).
std::vector<Engine::Rect> Engine::owner_tile_rects(int from, int to, int world) const {
    std::vector<Rect> out;
    if (from == to) return out;
    const int64_t o = no, ov = o * nv, npp = static_cast<int64_t>(nv) * (nv + 1) / 2;
    int64_t q0, q1, r0, r1;
    chunk(npp, to, world, q0, q1);
    if (q1 <= q0) return out;
    const int64_t A0 = static_cast<int64_t>(a_of_pair_row(q0)) * o, A1 = static_cast<int64_t>(a_of_pair_row(q1 - 1) + 1) * o;
    chunk(ov, from, world, r0, r1);
    if (std::min(r1, A1) > r0) out.push_back(Rect{r0, std::min(r1, A1), A0, A1});
    if (A0 > 0 && std::min(r1, A1) > std::max(r0, A0)) out.push_back(Rect{std::max(r0, A0), std::min(r1, A1), 0, A0});
    return out;
}
void Engine::owner_tile_sizes(int rank, int world, int64_t* send_doubles, int64_t* recv_doubles) const {
    if (world < 1 || rank < 0 || rank >= world) throw Error("owner_tile_sizes: bad rank/world");
    int64_t s = 0, r = 0;
    for (int q = 0; q < world; ++q) {
        for (const Rect& x : owner_tile_rects(rank, q, world)) s += 2 * (x.r1 - x.r0) * (x.c1 - x.c0);      // both matrices
        for (const Rect& x : owner_tile_rects(q, rank, world)) r += 2 * (x.r1 - x.r0) * (x.c1 - x.c0);
    }
    if (send_doubles) *send_doubles = std::max<int64_t>(s, 1);
    if (recv_doubles) *recv_doubles = std::max<int64_t>(r, 1);
}
int64_t Engine::owner_tiles_start(const ShardBuffers& b) {
    if (!alltoallv_ || !xs_ || !xr_) throw Error("sharded step: owner tiles need pymes_set_alltoallv and pymes_set_owner_tile_buffers");
    const int rank = coll_.rank, world = coll_.world;
    const int64_t ov = static_cast<int64_t>(no) * nv;
    std::vector<int64_t> ns(world, 0), nr(world, 0);
    int64_t off = 0;
    for (int q = 0; q < world; ++q)
        for (double* m : {b.ETd, b.ETx})
            for (const Rect& x : owner_tile_rects(rank, q, world)) {         // (small strided copies: tasks of ONE phase level)
                const int64_t rows = x.r1 - x.r0, cols = x.c1 - x.c0;
                copy(slice(slice(make_view(m, {x.r1, ov}), 0, x.r0, x.r1), 1, x.c0, x.c1), make_view(xs_ + off, {rows, cols}));
                off += rows * cols;
                ns[q] += rows * cols;
            }
    for (int p = 0; p < world; ++p)
        for (const Rect& x : owner_tile_rects(p, rank, world)) nr[p] += 2 * (x.r1 - x.r0) * (x.c1 - x.c0);
    dev::gemm_group_sync();
    dev::phase_sync();
    int64_t t = 0;
    if (alltoallv_(coll_.user, xs_, ns.data(), xr_, nr.data(), stream, &t) != 0) throw Error("collective hook: alltoallv_start failed");
    return t;
}
void Engine::owner_tiles_finish(const ShardBuffers& b) {
    const int rank = coll_.rank, world = coll_.world;
    const int64_t ov = static_cast<int64_t>(no) * nv;
    int64_t off = 0;
    for (int p = 0; p < world; ++p)
        for (double* m : {b.ETd, b.ETx})
            for (const Rect& x : owner_tile_rects(p, rank, world)) {
                const int64_t rows = x.r1 - x.r0, cols = x.c1 - x.c0;
                copy(make_view(xr_ + off, {rows, cols}), slice(slice(make_view(m, {x.r1, ov}), 0, x.r0, x.r1), 1, x.c0, x.c1));
                off += rows * cols;
            }
}

void Engine::ccsd_sharded_await(double* t2, const ShardBuffers& b) {
    if (!t2_in_flight_) return;
    if (!coll_set_) throw Error("sharded step: no collectives set (pymes_set_collectives)");
    const Hooks h{coll_, stream};
    h.wait(t2_ticket_);
    t2_in_flight_ = false;
    const int64_t o2 = static_cast<int64_t>(no) * no, c = chunk_of(static_cast<int64_t>(nv) * (nv + 1) / 2, coll_.world);
    for (int r = 0; r < coll_.world; ++r) {          // chunk r of the exchanged buffer: the compact tiles of rank r's pairs
        int64_t r0, r1;
        pair_chunk(r, coll_.world, r0, r1);
        dev::pairs_unpack(b.Tall + static_cast<int64_t>(r) * c * 2 * o2, t2, no, nv, r0, r1, stream);
    }
}

void Engine::ccsd_sharded_residuals(const double* f, double* fd, const double* t1, double* t2, const ShardBuffers& b,
                                    unsigned flags, double* rc) {
    if (!coll_set_) throw Error("sharded step: no collectives set (pymes_set_collectives)");
    if (!dev::fused_pair_kernels_ok(no)) throw Error("sharded step: nocc too large for the pair-sharded tail");
    const Hooks h{coll_, stream};
    const int rank = coll_.rank, world = coll_.world;
    check_shard_rank("ccsd_sharded_residuals", rank, world);
    const int64_t o = no, v = nv, ov = o * v, o2 = o * o;
    const unsigned dcd = flags & PYMES_DCD;
    const unsigned slab = dcd | PYMES_USE_DRESSED | PYMES_SYM_LADDER | PYMES_SYM_RINGS;
    const bool owner = (flags & PYMES_OWNER_TILES) != 0;
    h.mark("begin");
    // K-sharded partial sums, all-reduced: the T1.V intermediates of the dressed Fock matrix (ccsd.py:163, this rank's chunk of
    // j).  What needs T1 only comes first: the all-gather of the new T2 that the previous pass left in flight is awaited — and
    // unpacked into the replicated array — right before the first kernel that reads T2.
    dress_fock_partial(t1, b.W, rank, world);
    const int64_t tW = h.allreduce(b.W, dress_fock_ws_doubles());
    {
        // V~_iajb / V~_iabj only for the second-index range that this rank's column slab reads (:165); V~_klij rides in the
        // same call and shares its V_klcd t_dj intermediate with V~_iabj
        int64_t c0, c1;
        chunk(ov, rank, world, c0, c1);
        if (c1 > c0) {
            const int64_t cut[4] = {0, 0, c0 / o, (c1 + o - 1) / o};
            dress_V(t1, (1u << P_klij) | (1u << P_iajb) | (1u << P_iabj), cut);
        } else {
            dress_V(t1, 1u << P_klij);
        }
    }
    h.mark("T1-only: fock partial, dress V slab");
    ccsd_sharded_await(t2, b);
    slab_prepare(t2, b.P, rank, world, dcd);
    // P = [ X'_ki (o^2 doubles: read by the ring half) | pair-packed 2 V_klcd T_cdij (read by the ladder half) ]: two
    // all-reduces, the big one is awaited only in front of the ladders — behind the ring products
    const int64_t tX = h.allreduce(b.P, o2);
    const int64_t tJ = h.allreduce(b.P + o2, slab_prepare_ws_doubles() - o2);
    h.wait(tW);
    h.wait(tX);
    dress_fock_finish(f, t1, b.W, fd);
    h.mark("await T2, slab prepare, fock finish");
    // :171 in two halves: the ring products first, so that the all-gathers of their rows fly while the ladders — whose rows
    // of L never leave the rank — and the singles residual are computed
    residual_slab(fd, t2, b.ETd, b.ETx, b.L, rank, world, slab | PYMES_SLAB_RINGS_ONLY, t1, b.QK, b.P);
    h.mark("ring products");
    // rows of the ring products: two all-gathers of the whole matrices, or ONE all-to-all of the tiles each pair owner reads
    int64_t tD = 0, tE = 0, tO = 0;
    if (owner) tO = owner_tiles_start(b);
    else {
        tD = h.allgather(b.ETd, chunk_of(ov, world) * ov);
        tE = h.allgather(b.ETx, chunk_of(ov, world) * ov);
    }
    h.wait(tJ);
    residual_slab(fd, t2, b.ETd, b.ETx, b.L, rank, world, slab | PYMES_SLAB_LADDERS_ONLY, t1, b.QK, b.P);
    h.mark("ladders, Q_kb");
    const int64_t tQ = h.allgather(b.QK, chunk_of(ov, world) * o2);
    xvv_partial(fd, t2, b.Xvv, rank, world, dcd);                     // X_ac (ccd.py:206-221) over this rank's chunk of k
    const int64_t tV = h.allreduce(b.Xvv, v * v);
    singles_residual_partial(fd, t1, t2, b.R1, rank, world, true);    // :167 over this rank's chunk of the occupied index
    const int64_t tR = h.allreduce(b.R1, v * o);
    if (owner) {
        h.wait(tO);
        owner_tiles_finish(b);
    } else {
        h.wait(tD);
        h.wait(tE);
    }
    for (int64_t t : {tQ, tV, tR}) h.wait(t);
    h.mark("X_ac, singles residual, waits");
    int64_t r0, r1;
    pair_chunk(rank, world, r0, r1);
    if (r1 <= r0) dev::memset_zero(rc, sizeof(double) * 2 * o2, stream);       // a rank without pairs: one zero tile pair
    residual_finish_pairs(fd, t2, b.ETd, b.ETx, b.L, rc, slab, t1, b.QK, rank, world, b.Xvv);     // :171, this rank's pairs
    h.mark("finish + assembly (pairs)");
}

void Engine::ccd_sharded_residuals(const double* f, double* t2, const ShardBuffers& b, unsigned flags, double* rc) {
    if (!coll_set_) throw Error("sharded step: no collectives set (pymes_set_collectives)");
    if (!dev::fused_pair_kernels_ok(no)) throw Error("sharded step: nocc too large for the pair-sharded tail");
    const Hooks h{coll_, stream};
    const int rank = coll_.rank, world = coll_.world;
    check_shard_rank("ccd_sharded_residuals", rank, world);
    const int64_t o = no, v = nv, ov = o * v, o2 = o * o;
    const unsigned slab = (flags & PYMES_DCD) | PYMES_SYM_LADDER | PYMES_SYM_RINGS;   // undressed blocks: CCD / DCD have no T1 (ccd.py:100-121)
    const bool owner = (flags & PYMES_OWNER_TILES) != 0;
    h.mark("begin");
    ccsd_sharded_await(t2, b);                                 // the new T2 the previous pass left in flight
    residual_slab(f, t2, b.ETd, b.ETx, b.L, rank, world, slab | PYMES_SLAB_RINGS_ONLY);
    h.mark("ring products");
    int64_t tD = 0, tE = 0, tO = 0;
    if (owner) tO = owner_tiles_start(b);
    else {
        tD = h.allgather(b.ETd, chunk_of(ov, world) * ov);
        tE = h.allgather(b.ETx, chunk_of(ov, world) * ov);
    }
    residual_slab(f, t2, b.ETd, b.ETx, b.L, rank, world, slab | PYMES_SLAB_LADDERS_ONLY);      // the rows of L stay on the rank
    if (owner) {
        h.wait(tO);
        owner_tiles_finish(b);
    } else {
        h.wait(tD);
        h.wait(tE);
    }
    h.mark("ladders, waits");
    int64_t r0, r1;
    pair_chunk(rank, world, r0, r1);
    if (r1 <= r0) dev::memset_zero(rc, sizeof(double) * 2 * o2, stream);
    residual_finish_pairs(f, t2, b.ETd, b.ETx, b.L, rc, slab, nullptr, nullptr, rank, world, nullptr);
    h.mark("finish + assembly (pairs)");
}

int Engine::ccsd_sharded_finish(const double* f, const double* t1, const double* tc, const double* dtc, const ShardBuffers& b) {
    if (!coll_set_) throw Error("sharded step: no collectives set (pymes_set_collectives)");
    if (t2_in_flight_) throw Error("sharded step: the previous exchange of the amplitudes was never awaited");
    const Hooks h{coll_, stream};
    const int rank = coll_.rank, world = coll_.world;
    const int64_t o2 = static_cast<int64_t>(no) * no;
    int64_t r0, r1;
    pair_chunk(rank, world, r0, r1);
    const int64_t c = chunk_of(static_cast<int64_t>(nv) * (nv + 1) / 2, world);
    if (r1 > r0)
        dev::memcpy_d2d(b.Tall + static_cast<int64_t>(rank) * c * 2 * o2, tc, sizeof(double) * (r1 - r0) * 2 * o2, stream);
    // the energy and the norms (:189-197) come from the compact tiles: six partial sums, all-reduced where they are and copied
    // to the host on the side — nothing on this stream waits for the host.  The all-gather of the new T2 is only STARTED, after
    // that small all-reduce (a communicator runs its collectives in order: behind the 0.8-GB transfer the six numbers would
    // wait for it)
    dev::energy_norms_pairs_dev(f, t1, tc, get_static("Edir"), get_static("Eex"), dtc, no, nv, r0, r1, rank == 0 && t1 && f, b.S,
                                stream);
    h.wait(h.allreduce(b.S, 6));
    const int slot = dev::readback_start(b.S, 6, stream);
    t2_ticket_ = h.allgather(b.Tall, c * 2 * o2);
    t2_in_flight_ = true;
    h.mark("energy + norms (pairs)");
    return slot;
}

void Engine::ccsd_sharded_energy(int slot, double out[6]) {
    double r[6];
    dev::readback_wait(slot, r, 6);
    out[0] = 2.0 * r[0];
    out[1] = 2.0 * r[1];
    out[2] = -1.0 * r[2];
    out[3] = r[3];
    out[4] = r[4];
    out[5] = r[5];
}

void Engine::release_residual_buffers() {
    //  recorded graphs of ANY solver on this context replay into these buffers: they go back to the scratch pool —
    // where a later request of the same size would alias them — only when the last recorded graph is gone (graph_destroy)
    if (!graphs_.empty()) {
        release_wanted_ = true;
        return;
    }
    release_wanted_ = false;
    for (double** p : {&res_fd_, &res_ETd_, &res_ETx_, &res_L_, &res_QK_, &res_r1_, &res_r2_}) {
        if (*p) scratch_put(*p);
        *p = nullptr;
    }
}

void Engine::cc_update_to(double* t_out, double* dt, const double* t_in, const double* r, double shift, double delta,
                          int rank, bool sym) {
    if (rank != 2 && rank != 4) throw Error("cc_update: rank must be 2 (T1) or 4 (T2)");
    need_eps("cc_update");
    if (sym && rank == 4 && sym_tail()) dev::cc_update_to_sym(t_out, dt, t_in, r, eps_o, eps_v, shift, delta, no, nv, stream);
    else dev::cc_update_to(t_out, dt, t_in, r, eps_o, eps_v, shift, delta, no, nv, rank, stream);
}

void Engine::dots(int npairs, const double* const* x, const double* const* y, const int64_t* n, const int* sym, double* out) {
    bool any = false;
    for (int i = 0; sym && i < npairs && i < 16; ++i) any = any || sym[i];
    if (any && sym_tail()) dev::dots_sym(npairs, x, y, n, sym, no, nv, out, stream);
    else dev::dots(npairs, x, y, n, out, stream);
}

void Engine::lincomb(double* out, int nx, const double* const* x, const double* c, int64_t n, bool sym) {
    if (sym && n != (int64_t)nv * nv * no * no) throw Error("lincomb: a symmetric vector must be a [v,v,o,o] array");
    if (sym && sym_tail()) dev::lincomb_sym(out, nx, x, c, no, nv, stream);
    else dev::lincomb(out, nx, x, c, n, stream);
}

int Engine::energy_norms_start(const double* f, const double* t1, const double* t2, const double* dt2, bool sym) {
    if (sym && sym_tail()) return dev::energy_norms_start_sym(f, t1, t2, get_static("Edir"), get_static("Eex"), dt2, no, nv, stream);
    return dev::energy_norms_start(f, t1, t2, get_static("Edir"), get_static("Eex"), dt2, no, nv, stream);
}
void Engine::energy_norms_wait(int slot, double out[6]) {
    double r[6];
    dev::readback_wait(slot, r, 6);
    out[0] = 2.0 * r[0];
    out[1] = 2.0 * r[1];
    out[2] = -1.0 * r[2];
    out[3] = r[3];
    out[4] = r[4];
    out[5] = r[5];
}

void Engine::energy_norms(const double* f, const double* t1, const double* t2, const double* dt2, double out[6], bool sym) {
    if (sym && sym_tail()) return energy_norms_wait(energy_norms_start(f, t1, t2, dt2, true), out);
    double r[6];
    dev::energy_norms(f, t1, t2, get_static("Edir"), get_static("Eex"), dt2, no, nv, r, stream);
    out[0] = 2.0 * r[0];      // ccsd.py:465
    out[1] = 2.0 * r[1];      // :463 / ccd.py:260
    out[2] = -1.0 * r[2];     // :464 / ccd.py:261
    out[3] = r[3];
    out[4] = r[4];
    out[5] = r[5];
}

// the same over the compact tiles of this rank's pairs (one process per GPU): partial sums, to be all-reduced; the T1
// terms enter on rank 0
void Engine::energy_norms_pairs(const double* f, const double* t1, const double* tc, const double* dtc, int rank, int world,
                                double out[6]) {
    int64_t r0, r1;
    pair_chunk(rank, world, r0, r1);
    double r[6];
    dev::energy_norms_pairs(f, t1, tc, get_static("Edir"), get_static("Eex"), dtc, no, nv, r0, r1, rank == 0, r, stream);
    out[0] = 2.0 * r[0];
    out[1] = 2.0 * r[1];
    out[2] = -1.0 * r[2];
    out[3] = r[3];
    out[4] = r[4];
    out[5] = r[5];
}

void Engine::ccsd_energy(const double* f, const double* t1, const double* t2, double out[3]) {
    double r[6];
    energy_norms(f, t1, t2, nullptr, r);
    out[0] = r[0];
    out[1] = r[1];
    out[2] = r[2];
}

void Engine::ccd_energy(const double* t2, double out[2]) {
    double r[6];
    energy_norms(nullptr, nullptr, t2, nullptr, r);
    out[0] = r[1];
    out[1] = r[2];
}

// -----------------------------------------------------------------------------------
// integral sharding (pymes_set_integral_shard): V_abcd exists only as this rank's rows of its pair-packed form
// -----------------------------------------------------------------------------------
namespace {
// bytes of the one staging buffer through which a host (or device) V_pqrs reaches the device in sharded mode
int64_t shard_staging_bytes() {
    if (const char* e = getenv("PYMES_SHARD_STAGING_BYTES")) {
        const long long b = atoll(e);
        if (b > 0) return b;
    }
    return int64_t(1) << 30;
}
}

void Engine::set_integral_shard(int rank, int world) {
    if (world < 1 || rank < 0 || rank >= world) throw Error("integral shard: need 0 <= rank < world");
    if (shard_on_) throw Error("the context already shards its integrals");
    refuse_if_direct("pymes_set_integral_shard");
    for (int p = 0; p < 16; ++p)
        if (V_[p] || Vd_[p]) throw Error("pymes_set_integral_shard must be called before any pymes_set_V_* call");
    shard_on_ = true;
    shard_rank_ = rank;
    shard_world_ = world;
    pair_chunk(rank, world, srows_.row0, srows_.row1);
}

void Engine::refuse_if_sharded(const char* who) const {
    if (!shard_on_) return;
    throw Error(std::string(who) + ": not available with integral sharding (pymes_set_integral_shard, rank " +
                std::to_string(shard_rank_) + " of " + std::to_string(shard_world_) +
                "): the context holds only its rows of the pair-packed V_abcd, not the full or dressed block");
}

void Engine::check_shard_rank(const char* who, int rank, int world) const {
    if (shard_on_ && (rank != shard_rank_ || world != shard_world_))
        throw Error(std::string(who) + ": rank " + std::to_string(rank) + " of " + std::to_string(world) +
                    " does not match the integral shard of this context (rank " + std::to_string(shard_rank_) + " of " +
                    std::to_string(shard_world_) + ")");
}

void Engine::check_shard_rows(const char* who, int64_t row0, int64_t row1, bool dressed) const {
    if (dressed) refuse_if_sharded((std::string(who) + " with the dressed V_abcd").c_str());
    if (row0 != srows_.row0 || row1 != srows_.row1)
        throw Error(std::string(who) + ": pair rows [" + std::to_string(row0) + "," + std::to_string(row1) +
                    ") are not the rows [" + std::to_string(srows_.row0) + "," + std::to_string(srows_.row1) +
                    ") that this context holds (integral sharding, rank " + std::to_string(shard_rank_) + " of " +
                    std::to_string(shard_world_) + ")");
    if (!srows_.set) throw Error(std::string(who) + ": the rows of V_abcd have not been set (integral sharding)");
}

void Engine::shard_rows(const double** vp, const double** vm, int64_t* row0, int64_t* row1, int64_t* ldp, int64_t* ldm) const {
    if (!shard_on_) throw Error("pymes_shard_rows_ptr: the context does not shard its integrals");
    if (!srows_.set) throw Error("pymes_shard_rows_ptr: the rows of V_abcd have not been set");
    *vp = srows_.Vp;
    *vm = srows_.Vm;
    *row0 = srows_.row0;
    *row1 = srows_.row1;
    *ldp = pair_dims().vlp;
    *ldm = pair_dims().vlm;
}

void Engine::shard_rows_alloc() {
    const int64_t rows = srows_.row1 - srows_.row0;
    if (srows_.Vp || rows <= 0) return;
    srows_.Vp = static_cast<double*>(dev::dmalloc(sizeof(double) * rows * pair_dims().vlp));
    srows_.Vm = static_cast<double*>(dev::dmalloc(sizeof(double) * rows * pair_dims().vlm));
}

int64_t Engine::integral_bytes() const {
    const int64_t lp = pair_dims().vlp, lm = pair_dims().vlm;
    int64_t d = 0;
    for (int p = 0; p < 16; ++p) d += (V_[p] ? block_size(p) : 0) + (Vd_[p] ? block_size(p) : 0);
    for (auto& kv : static_doubles_) d += kv.second;
    if (lpack_.Vp) d += (lpack_.row1 - lpack_.row0) * (lp + lm);
    if (srows_.Vp) d += (srows_.row1 - srows_.row0) * (lp + lm);
    if (direct_.Bvv) d += nv * direct_.qp * direct_.xp;
    if (direct_.Vp) d += direct_.cap * (lp + lm);
    if (direct_.planes) d += direct_.prow * nv * nv;
    return d * static_cast<int64_t>(sizeof(double));
}

// -----------------------------------------------------------------------------------
// factor-direct particle ladder (pymes_set_integral_direct): nothing of size v^4 exists; the rows of the pair-packed V_abcd
// are rebuilt from the virtual-virtual factors chunk by chunk inside every ladder call
// -----------------------------------------------------------------------------------
void Engine::set_integral_direct(int64_t chunk_bytes) {
    if (chunk_bytes < 0) throw Error("pymes_set_integral_direct: chunk_bytes must be >= 0 (0: PYMES_DIRECT_CHUNK_BYTES, default 1 GiB)");
    if (direct_.on) throw Error("the context is already factor-direct (pymes_set_integral_direct)");
    refuse_if_sharded("pymes_set_integral_direct");
    for (int p = 0; p < 16; ++p)
        if (V_[p] || Vd_[p]) throw Error("pymes_set_integral_direct must be called before any pymes_set_V_* call");
    if (chunk_bytes == 0) {
        chunk_bytes = int64_t(1) << 30;
        if (const char* e = getenv("PYMES_DIRECT_CHUNK_BYTES")) {
            const long long b = atoll(e);
            if (b > 0) chunk_bytes = b;
        }
    }
    // the row builder: PYMES_DIRECT_BUILDER=gemm|fused; without it the fused kernel where the backend has it (every fused run
    // was below every gemm run in profiles/direct/probe_direct.txt), else the gemm route
    bool fused = dev::direct_rows_fused_ok();
    if (const char* e = getenv("PYMES_DIRECT_BUILDER")) {
        const std::string b(e);
        if (b == "fused") {
            if (!dev::direct_rows_fused_ok())
                throw Error("PYMES_DIRECT_BUILDER=fused: the fused row builder of the factor-direct mode is not available in this backend");
            fused = true;
        } else if (b == "gemm") {
            fused = false;
        } else {
            throw Error("PYMES_DIRECT_BUILDER must be gemm or fused (factor-direct mode, pymes_set_integral_direct)");
        }
    }
    direct_.on = true;
    direct_.fused = fused;
    direct_.chunk_bytes = chunk_bytes;
}

void Engine::refuse_if_direct(const char* who) const {
    if (!direct_.on) return;
    throw Error(std::string(who) + ": not available on a factor-direct context (pymes_set_integral_direct): it holds the "
                "virtual-virtual factors and rebuilds the undressed pair-packed rows of V_abcd chunk by chunk, never the full, "
                "dressed or stored block");
}

// B_vv [nv][qp][xp] (device_api.h, direct_rows_fused) from the factors on the device, and the chunk buffers: cap rows of
// V^+ / V^- at the ladder pitches and, for the gemm builder, as many planes V[a,b,:,:] — all within chunk_bytes (at least one row).
void Engine::direct_setup(const double* Bd, int naux) {
    const PairDims d = pair_dims();
    const int64_t v = nv, nn = n, rowb = 8 * (d.vlp + d.vlm), planeb = 8 * v * v;
    dev::stream_sync(stream);
    for (double** p : {&direct_.Bvv, &direct_.Vp, &direct_.Vm, &direct_.planes}) {
        dev::dfree(*p);
        *p = nullptr;
    }
    direct_.naux = naux;
    direct_.qp = (int64_t(naux) + 7) & ~int64_t(7);
    direct_.xp = (v + 63) & ~int64_t(63);
    direct_.cap = std::max<int64_t>(1, std::min<int64_t>(d.npp, direct_.chunk_bytes / (rowb + (direct_.fused ? 0 : planeb))));
    direct_.prow = direct_.fused ? 0 : direct_.cap;
    const int64_t bsz = v * direct_.qp * direct_.xp;
    direct_.Bvv = static_cast<double*>(dev::dmalloc(sizeof(double) * bsz));
    direct_.Vp = static_cast<double*>(dev::dmalloc(sizeof(double) * direct_.cap * d.vlp));
    direct_.Vm = static_cast<double*>(dev::dmalloc(sizeof(double) * direct_.cap * d.vlm));
    if (direct_.prow) direct_.planes = static_cast<double*>(dev::dmalloc(sizeof(double) * direct_.prow * v * v));
    dev::memset_zero(direct_.Bvv, sizeof(double) * bsz, stream);
    const int64_t dims[3] = {naux, v, v}, sst[3] = {nn * nn, nn, 1}, dst[3] = {direct_.xp, direct_.qp * direct_.xp, 1};
    permute(1.0, make_view(const_cast<double*>(Bd) + no * nn + no, 3, dims, sst), "Qax", 0.0, make_view(direct_.Bvv, 3, dims, dst), "Qax");
}

void Engine::direct_build(int64_t c0, int64_t c1, int builder) {
    const PairDims d = pair_dims();
    const int64_t v = nv, plane = v * v, pa = direct_.qp * direct_.xp;
    if (!direct_.Bvv) throw Error("factor-direct context: the integrals have not been set (pymes_set_V_from_factors)");
    if (c0 < 0 || c1 > d.npp || c0 >= c1 || c1 - c0 > direct_.cap) throw Error("factor-direct context: bad chunk of pair rows");
    const bool fused = builder < 0 ? direct_.fused : builder == 1;
    if (fused) {
        dev::direct_rows_fused(direct_.Bvv, direct_.Vp, direct_.Vm, nv, direct_.qp, direct_.xp, c0, c1, stream, d.vlp, d.vlm);
        return;
    }
    if (!direct_.planes) throw Error("factor-direct context: the gemm builder needs its planes buffer (PYMES_DIRECT_BUILDER=gemm at set-up)");
    // planes[r - c0][c][d] = sum_Q B_vv[a][Q][c] B_vv[b][Q][d] = V_abcd for the rows r = P(a,b) of the chunk: one batched product
    // per a (consecutive b are consecutive rows); V_abdc is the transposed plane, so nothing is computed twice
    for (int64_t r = c0; r < c1;) {
        const int64_t a = a_of_pair_row(r), b = r - a * (a + 1) / 2;
        const int64_t nb = std::min(c1, (a + 1) * (a + 2) / 2) - r;
        const int64_t ad[2] = {direct_.naux, v}, as[2] = {direct_.xp, 1};
        const int64_t bd[3] = {nb, direct_.naux, v}, bs[3] = {pa, direct_.xp, 1};
        contract(1.0, make_view(direct_.Bvv + a * pa, 2, ad, as), "Qc", make_view(direct_.Bvv + b * pa, 3, bd, bs), "bQd", 0.0,
                 make_view(direct_.planes + (r - c0) * plane, {nb, v, v}), "bcd", "b");
        r += nb;
    }
    dev::gemm_group_sync();
    // (the nr == 0 form of ladder_pack_V takes row r from V + r plane and packs every row as it is: the V^- rows of the pairs
    // a == b, zero in the [nr,nr,nc,nc] form, are cleared afterwards as shard_rows_from does)
    dev::ladder_pack_V(direct_.planes - c0 * plane, direct_.Vp, direct_.Vm, 0, nv, c0, c1, stream, d.vlp, d.vlm);
    for (int64_t a = a_of_pair_row(c0); a < v; ++a) {
        const int64_t r = a * (a + 3) / 2;
        if (r >= c1) break;
        if (r >= c0) dev::memset_zero(direct_.Vm + (r - c0) * d.vlm, sizeof(double) * d.vlm, stream);
    }
}

void Engine::direct_ladder_products(int64_t row0, int64_t row1, const TView& SpT, const TView& AmT, const TView& LS,
                                    const TView& LA) {
    const PairDims d = pair_dims();
    dev::gemm_group_sync();            // (the chunk buffers are rewritten below: nothing that reads them may still be queued)
    for (int64_t c0 = row0; c0 < row1; c0 += direct_.cap) {
        const int64_t c1 = std::min(row1, c0 + direct_.cap), m = c1 - c0;
        direct_build(c0, c1);
        GemmGroupScope grp(stream);
        contract(1.0, packed_rows(direct_.Vp, m, d.npp), "rk", SpT, "kn", 0.0, slice(LS, 0, c0 - row0, c1 - row0), "rn");
        if (d.opm > 0 && d.npm > 0)
            contract(1.0, packed_rows(direct_.Vm, m, d.npm), "rk", AmT, "kn", 0.0, slice(LA, 0, c0 - row0, c1 - row0), "rn");
        grp.close();
    }
}

void Engine::direct_info(int64_t out[5]) const {
    if (!direct_.on) throw Error("pymes_direct_info: the context is not factor-direct (pymes_set_integral_direct)");
    const PairDims d = pair_dims();
    out[0] = direct_.naux;
    out[1] = direct_.cap;
    out[2] = direct_.Bvv ? 8 * nv * direct_.qp * direct_.xp : 0;
    out[3] = direct_.Vp ? 8 * (direct_.cap * (d.vlp + d.vlm) + direct_.prow * nv * nv) : 0;
    out[4] = direct_.fused ? 1 : 0;
}

void Engine::direct_rows(int64_t r0, int64_t r1, const double** vp, const double** vm, int64_t* ldp, int64_t* ldm) {
    if (!direct_.on) throw Error("pymes_direct_rows: the context is not factor-direct (pymes_set_integral_direct)");
    if (capturing_) throw Error("pymes_direct_rows while a launch graph is being recorded");
    direct_build(r0, r1);
    dev::stream_sync(stream);
    *vp = direct_.Vp;
    *vm = direct_.Vm;
    *ldp = pair_dims().vlp;
    *ldm = pair_dims().vlm;
}

// The planes V[a,b,:,:] of this rank's pair rows (V0: the element V[0,0,0,0] of the virtual block, strides st), gathered in
// pair order — consecutive b of one a are one strided copy — into the staging buffer chunk by chunk and packed by
// ladder_pack_V in its nr == 0 form (the rows of the chunk are consecutive planes).
void Engine::shard_rows_from(const double* V0, const int64_t st[4], bool on_device) {
    shard_rows_alloc();
    const int64_t v = nv, plane = v * v, lp = pair_dims().vlp, lm = pair_dims().vlm;
    const int64_t r0 = srows_.row0, r1 = srows_.row1;
    srows_.set = false;
    if (r1 > r0) {
        const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(r1 - r0, shard_staging_bytes() / (8 * plane)));
        std::vector<double> host(on_device ? 0 : cap * plane);
        double* stage = static_cast<double*>(dev::dmalloc(sizeof(double) * cap * plane));
        try {
            for (int64_t c0 = r0; c0 < r1; c0 += cap) {
                const int64_t c1 = std::min(r1, c0 + cap);
                for (int64_t r = c0; r < c1;) {
                    const int64_t a = a_of_pair_row(r), b = r - a * (a + 1) / 2;
                    const int64_t nb = std::min(c1, (a + 1) * (a + 2) / 2) - r;          // planes (a,b) .. (a,b+nb-1)
                    const double* src = V0 + a * st[0] + b * st[1];
                    if (on_device) {
                        const int64_t dims[3] = {nb, v, v}, sst[3] = {st[1], st[2], st[3]};
                        copy(make_view(const_cast<double*>(src), 3, dims, sst), make_view(stage + (r - c0) * plane, {nb, v, v}));
                    } else {
                        double* dst = host.data() + (r - c0) * plane;
                        for (int64_t q = 0; q < nb; ++q)
                            for (int64_t c = 0; c < v; ++c) {
                                const double* row = src + q * st[1] + c * st[2];
                                double* out = dst + (q * v + c) * v;
                                if (st[3] == 1) std::memcpy(out, row, sizeof(double) * v);
                                else for (int64_t d = 0; d < v; ++d) out[d] = row[d * st[3]];
                            }
                    }
                    r += nb;
                }
                if (!on_device) dev::memcpy_h2d(stage, host.data(), sizeof(double) * (c1 - c0) * plane, stream);
                dev::ladder_pack_V(stage - c0 * plane, srows_.Vp + (c0 - r0) * lp, srows_.Vm + (c0 - r0) * lm, 0, nv, c0, c1,
                                   stream, lp, lm);
                dev::stream_sync(stream);            // the staging buffers are refilled next
            }
        } catch (...) {
            dev::dfree(stage);
            throw;
        }
        dev::dfree(stage);
        // the nr == 0 form packs every row as it is: the V^- rows of the pairs a == b are zero in the [nr,nr,nc,nc] form
        for (int64_t a = 0; a < v; ++a) {
            const int64_t r = a * (a + 3) / 2;
            if (r >= r0 && r < r1) dev::memset_zero(srows_.Vm + (r - r0) * lm, sizeof(double) * lm, stream);
        }
        dev::stream_sync(stream);
    }
    srows_.set = true;
}

void Engine::shard_rows_from_factors(const double* Bd, int naux) {
    shard_rows_alloc();
    const int64_t lp = pair_dims().vlp, lm = pair_dims().vlm;
    srows_.set = false;
    if (srows_.row1 > srows_.row0)
        dev::ladder_pack_V_factors(Bd, srows_.Vp, srows_.Vm, naux, n, no, srows_.row0, srows_.row1, stream, lp, lm);
    srows_.set = true;
}

// V_pqrs without staging n^4 on the device: the 15 blocks other than V_abcd (host: gathered in slices of their first index
// through a bounded host buffer, uploaded into their own storage; device: strided copies as in set_V_full) and the rows
void Engine::set_V_full_sharded(const double* V, bool on_device, const int64_t strides[4]) {
    const int64_t nn = n;
    int64_t st[4] = {nn * nn * nn, nn * nn, nn, 1};
    if (on_device && strides)
        for (int i = 0; i < 4; ++i) st[i] = strides[i];
    std::vector<double> host;
    for (int pat = 0; pat < 15; ++pat) {
        if (!V_[pat]) V_[pat] = static_cast<double*>(dev::dmalloc(sizeof(double) * block_size(pat)));
        int64_t d[4], off = 0;
        for (int i = 0; i < 4; ++i) {
            const bool virt = pat >> (3 - i) & 1;
            d[i] = virt ? nv : no;
            if (virt) off += no * st[i];
        }
        const double* src = V + off;
        if (on_device) {
            TView sv = make_view(const_cast<double*>(src), 4, d, st);
            copy(sv, block_view(V_[pat], pat));
            continue;
        }
        const int64_t slice_el = d[1] * d[2] * d[3];
        const int64_t cap = std::max<int64_t>(1, std::min<int64_t>(d[0], shard_staging_bytes() / (8 * slice_el)));
        host.resize(static_cast<size_t>(cap * slice_el));
        for (int64_t i0 = 0; i0 < d[0]; i0 += cap) {
            const int64_t i1 = std::min(d[0], i0 + cap);
            double* out = host.data();
            for (int64_t i = i0; i < i1; ++i)
                for (int64_t j = 0; j < d[1]; ++j)
                    for (int64_t k = 0; k < d[2]; ++k, out += d[3])
                        std::memcpy(out, src + i * st[0] + j * st[1] + k * st[2], sizeof(double) * d[3]);
            dev::memcpy_h2d(V_[pat] + i0 * slice_el, host.data(), sizeof(double) * (i1 - i0) * slice_el, stream);
            dev::stream_sync(stream);
        }
    }
    shard_rows_from(V + no * (st[0] + st[1] + st[2] + st[3]), st, on_device);
}

// ---------------------------------------------------------------------------------
// (T) correction: include/pymes_amd.h, pymes_ccsd_t (the formulas there and in tests/_triples_reference.py)
// ---------------------------------------------------------------------------------
int64_t Engine::triples_count(int no) { return (int64_t)no * (no + 1) * (no + 2) / 6; }

namespace {
// device buffers of one ccsd_t call, released on every way out
struct DevBufs {
    std::vector<void*> p;
    double* get(int64_t doubles) {
        p.push_back(dev::dmalloc(sizeof(double) * std::max<int64_t>(doubles, 1)));
        return static_cast<double*>(p.back());
    }
    ~DevBufs() {
        for (void* q : p) dev::dfree(q);
    }
};
void unrank_triple(int64_t t, int& i, int& j, int& k) {
    int x = 0;
    while ((int64_t)(x + 1) * (x + 2) * (x + 3) / 6 <= t) ++x;
    int64_t r = t - (int64_t)x * (x + 1) * (x + 2) / 6;
    int y = 0;
    while ((int64_t)(y + 1) * (y + 2) / 2 <= r) ++y;
    i = x;
    j = y;
    k = (int)(r - (int64_t)y * (y + 1) / 2);
}
// The operands of the twelve products of one W_ijk: X1[p][f][x][y] and its swapped pair X1s[f][p][x][y] = X1[p][f][y][x]
// ([o,v,v,v], [v,o,v,v]), X2[p][q][x][m] ([o,o,v,o]) and the permuted amplitudes A2o[x][y][f][z] = A[z,f,x,y],
// A2h[m][k][b][c] = A[b,c,m,k] ([o,o,v,v]).  (T) and the left triples of Lambda-CCSD(T): V_iabc, V_aibc, V_ijak; the right
// triples: copies of V_abic and V_aijk in these layouts.
struct TriplesOperands {
    const double *X1, *X1s, *X2, *A2o, *A2h;
};
// Wq[a][b][c] = w_ijk[abc] + w_jik[bac] + w_ikj[acb] + w_kij[cab] + w_jki[bca] + w_kji[cba], each w_pqr[x,y,z] =
//   sum_f X1[p,f,x,y] A2o[r][q][f][z] - sum_m X2[p,q,x,m] A2h[m][r][y][z]
// written with the unit-stride index c as N: X1[p,f,y,x] = X1s[f,p,x,y] supplies the swapped pairs.  The same launches
// whatever else the caller holds: every sum has one order.
void triples_W(Engine& e, double* Wq, int i, int j, int k, const TriplesOperands& x) {
    const int64_t o = e.no, v = e.nv, v2 = v * v, v3 = v2 * v;
    const double *Viabc = x.X1, *Vaibc = x.X1s, *Vijak = x.X2, *T2o = x.A2o, *T2h = x.A2h;
    auto mm = [&](double* C, int64_t M, int64_t N, int64_t K, double alpha, double beta, const double* A, int64_t a_sm,
                  int64_t a_sk, const double* B, int64_t b_sk, int64_t b_sn, int64_t ldc, int64_t nb = 1, int64_t b_b = 0,
                  int64_t c_b = 0) {
        dev::Gemm g{};
        g.M = M; g.N = N; g.K = K;
        g.alpha = alpha; g.beta = beta;
        g.A = A; g.a_sm = a_sm; g.a_sk = a_sk;
        g.B = B; g.b_sk = b_sk; g.b_sn = b_sn;
        g.C = C; g.ldc = ldc;
        g.nb1 = nb; g.nb2 = 1;
        g.a_b1 = 0; g.b_b1 = b_b; g.c_b1 = c_b;
        g.a_b2 = g.b_b2 = g.c_b2 = 0;
        g.splitk_ws = nullptr;          // no k-split: the order of every sum is that of the tile kernel alone
        g.splitk_ws_doubles = 0;
        dev::gemm(g, e.stream);
        e.stats.gemm_calls++;
        e.stats.gemm_flops += 2.0 * (double)M * (double)N * (double)K * (double)nb;
    };
    // (the names are those of (T): Viabc = X1, Vaibc = X1s, Vijak = X2, T2o / T2h = A2o / A2h)
    // particle products (K = v)
    mm(Wq, v2, v, v, 1.0, 0.0, Viabc + i * v3, 1, v2, T2o + (k * o + j) * v2, v, 1, v);                 // w_ijk[a,b,c]
    mm(Wq, v2, v, v, 1.0, 1.0, Vaibc + j * v2, 1, o * v2, T2o + (k * o + i) * v2, v, 1, v);             // w_jik[b,a,c]
    mm(Wq, v, v, v, 1.0, 1.0, T2o + (j * o + k) * v2, 1, v, Viabc + i * v3, v2, 1, v, v, v, v2);       // w_ikj[a,c,b]
    mm(Wq, v, v, v, 1.0, 1.0, T2o + (j * o + i) * v2, 1, v, Vaibc + k * v2, o * v2, 1, v, v, v, v2);   // w_kij[c,a,b]
    mm(Wq, v, v2, v, 1.0, 1.0, T2o + (i * o + k) * v2, 1, v, Viabc + j * v3, v2, 1, v2);               // w_jki[b,c,a]
    mm(Wq, v, v2, v, 1.0, 1.0, T2o + (i * o + j) * v2, 1, v, Vaibc + k * v2, o * v2, 1, v2);           // w_kji[c,b,a]
    // hole products (K = o)
    mm(Wq, v, v2, o, -1.0, 1.0, Vijak + (i * o + j) * v * o, o, 1, T2h + k * v2, o * v2, 1, v2);       // w_ijk[a,b,c]
    mm(Wq, v, v2, o, -1.0, 1.0, Vijak + (i * o + k) * v * o, o, 1, T2h + j * o * v2, v2, 1, v2);       // w_ikj[a,c,b]
    mm(Wq, v, v, o, -1.0, 1.0, Vijak + (j * o + i) * v * o, o, 1, T2h + k * v2, o * v2, 1, v, v, v, v2);   // w_jik[b,a,c]
    mm(Wq, v, v, o, -1.0, 1.0, Vijak + (j * o + k) * v * o, o, 1, T2h + i * o * v2, v2, 1, v, v, v, v2);   // w_jki[b,c,a]
    mm(Wq, v2, v, o, -1.0, 1.0, T2h + j * v2, 1, o * v2, Vijak + (k * o + i) * v * o, 1, o, v);         // w_kij[c,a,b]
    mm(Wq, v2, v, o, -1.0, 1.0, T2h + i * o * v2, 1, v2, Vijak + (k * o + j) * v * o, 1, o, v);         // w_kji[c,b,a]
}
}  // namespace

void Engine::check_hermitian(const char* who, const char* why) {
    constexpr int P_aijk = 8;
    for (int pat : {P_iabc, P_abic, P_ijak, P_aijk})
        if (!V_[pat])
            throw Error(std::string(who) + " needs the undressed integral block '" + canonical_name(pat) + "', which has not been set");
    const int64_t o = no, v = nv, v2 = v * v, v3 = v2 * v;
    // Hermitian integrals (V_pqrs = V_rspq): V_iabc[i,a,b,c] = V_abic[b,c,i,a], V_ijak[i,j,a,k] = V_aijk[a,k,i,j].  The partner
    // is permuted into the [d1,d0,d3,d2] layout that dev::exchange_asymmetry compares against (max |A[p,q,r,s] - B[q,p,s,r]|).
    {
        DevBufs chk;
        double* Bt = chk.get(std::max(o * v3, o * o * o * v));     // holds either partner: [v,o,v,v] and [o,o,o,v]
        double worst = 0.0, vmax = 0.0;
        const char* what = "";
        permute(1.0, block(P_abic), "bcia", 0.0, make_view(Bt, {v, o, v, v}), "aicb");
        const int64_t d1[4] = {o, v, v, v};
        double r[2];
        dev::exchange_asymmetry(V_[P_iabc], Bt, d1, r, stream);
        worst = r[0]; vmax = r[1]; what = "V_iabc - V_abic";
        permute(1.0, block(P_aijk), "akij", 0.0, make_view(Bt, {o, o, o, v}), "jika");
        const int64_t d2[4] = {o, o, v, o};
        dev::exchange_asymmetry(V_[P_ijak], Bt, d2, r, stream);
        if (r[0] > worst) { worst = r[0]; what = "V_ijak - V_aijk"; }
        vmax = std::max(vmax, r[1]);
        if (!(worst <= 1e-10 * vmax)) {
            char buf[400];
            snprintf(buf, sizeof buf, "%s needs Hermitian integrals (V_pqrs = V_rspq): max |%s| = %.3e against max |V| = %.3e "
                     "(%s)", who, what, worst, vmax, why);
            throw Error(buf);
        }
    }
}

double Engine::ccsd_t(const double* eps_host, const double* t1, const double* t2, int64_t t_begin, int64_t t_end,
                      double* per_triple) {
    if (capturing_) throw Error("ccsd_t reads its energy back: not inside a launch graph");
    if (!eps_host) throw Error("ccsd_t: null pointer: eps");
    if (!t2) throw Error("ccsd_t: null pointer: t2");
    const int64_t ntot = triples_count(no);
    if (t_begin < 0 || t_end < t_begin || t_end > ntot)
        throw Error("ccsd_t: triple range [" + std::to_string(t_begin) + ", " + std::to_string(t_end) + ") outside [0, " +
                    std::to_string(ntot) + ")");
    constexpr int P_aijk = 8;
    // the UNDRESSED blocks only (a T1 dressing of the same context does not touch them)
    for (int pat : {P_iabc, P_aibc, P_ijak, P_abic, P_aijk})
        if (!V_[pat]) throw Error("ccsd_t needs the undressed integral block '" + canonical_name(pat) + "', which has not been set");
    if (t1 && !V_[P_ijab]) throw Error("ccsd_t needs the undressed integral block 'ijab', which has not been set");
    const int64_t o = no, v = nv, v2 = v * v, v3 = v2 * v;
    DevBufs bufs;
    check_hermitian("ccsd_t", "a transcorrelated Hamiltonian has no (T) here");
    if (t_end == t_begin) return 0.0;
    // the permuted amplitudes: T2o[x][y][f][z] = T[z,f,x,y] (particle products), T2h[m][k][b][c] = T[b,c,m,k] (hole products;
    // with T[c,b,m,j] = T[b,c,j,m], the exchange symmetry of CC amplitudes)
    double* T2o = bufs.get(o * o * v2);
    double* T2h = bufs.get(o * o * v2);
    const TView Tv = make_view(t2, {v, v, o, o});
    permute(1.0, Tv, "zfxy", 0.0, make_view(T2o, {o, o, v, v}), "xyfz");
    permute(1.0, Tv, "bcmk", 0.0, make_view(T2h, {o, o, v, v}), "mkbc");
    double* eps = bufs.get(n);
    dev::memcpy_h2d(eps, eps_host, sizeof(double) * n, stream);
    double* out = per_triple ? per_triple : bufs.get(t_end - t_begin);
    // batch: W of that many triples is held before one launch of the energy kernel.  Each W_ijk is built by products of its
    // own (the same launches whatever the batch), so the per-triple values do not depend on it.  Default: 128 MB of W, within a
    // quarter of the free memory (measured, DESIGN 7b: at (50,200) 8 triples per batch take 21.3 s against 20.1 s for this
    // default's 2; at (30,120) one triple per batch takes 4x as long, the energy launches under-fill the chip).
    int64_t batch = 0;
    if (const char* e = getenv("PYMES_TRIPLES_BATCH")) batch = atoll(e);
    if (batch <= 0) {
        const double budget = std::min(128.0 * (1 << 20), 0.25 * (double)dev::mem_free_bytes());
        batch = std::max<int64_t>(1, (int64_t)(budget / (8.0 * (double)v3)));
    }
    batch = std::min<int64_t>({batch, t_end - t_begin, 65535});
    double* W = bufs.get(batch * v3);
    double* partial = bufs.get(dev::triples_partial_doubles(nv, batch));
    const TriplesOperands ops{V_[P_iabc], V_[P_aibc], V_[P_ijak], T2o, T2h};
    for (int64_t t0 = t_begin; t0 < t_end; t0 += batch) {
        const int64_t nt = std::min(batch, t_end - t0);
        for (int64_t q = 0; q < nt; ++q) {
            int i, j, k;
            unrank_triple(t0 + q, i, j, k);
            triples_W(*this, W + q * v3, i, j, k, ops);
        }
        dev::triples_energy(W, nt, t0, t1 ? V_[P_ijab] : nullptr, t1, eps, partial, out + (t0 - t_begin), no, nv, stream);
    }
    // the sum over the range in a fixed order (the same whatever the batch)
    std::vector<double> h(t_end - t_begin);
    dev::memcpy_d2h(h.data(), out, sizeof(double) * h.size(), stream);
    dev::stream_sync(stream);
    double e = 0.0;
    for (double x : h) e += x;
    return e;
}

// ---- Lambda-CCSD(T): include/pymes_amd.h, pymes_ccsd_t_lambda (the formulas there and in tests/_lambda_triples_reference.py) ----
double Engine::ccsd_t_lambda(const double* eps_host, const double* t2, const double* lam1, const double* lam2, int64_t t_begin,
                             int64_t t_end, double* per_triple) {
    const char* who = "ccsd_t_lambda";
    if (capturing_) throw Error("ccsd_t_lambda reads its energy back: not inside a launch graph");
    if (!eps_host) throw Error("ccsd_t_lambda: null pointer: eps");
    if (!t2) throw Error("ccsd_t_lambda: null pointer: t2");
    if (!lam2) throw Error("ccsd_t_lambda: null pointer: lam2");
    const int64_t ntot = triples_count(no);
    if (t_begin < 0 || t_end < t_begin || t_end > ntot)
        throw Error("ccsd_t_lambda: triple range [" + std::to_string(t_begin) + ", " + std::to_string(t_end) + ") outside [0, " +
                    std::to_string(ntot) + ")");
    constexpr int P_aijk = 8;
    // the UNDRESSED blocks only: the five the products read, then their partners under (p,q,r,s) -> (q,p,s,r)
    for (int pat : {P_iabc, P_aibc, P_ijak, P_abic, P_aijk, P_ijka, P_abci, P_iajk})
        if (!V_[pat])
            throw Error("ccsd_t_lambda needs the undressed integral block '" + canonical_name(pat) + "', which has not been set");
    if (lam1 && !V_[P_ijab]) throw Error("ccsd_t_lambda needs the undressed integral block 'ijab', which has not been set");
    const int64_t o = no, v = nv, v2 = v * v, v3 = v2 * v;
    // V_pqrs = V_qpsr on what is read: the closed-shell formula rests on it (and on nothing else: no V_pqrs = V_rspq)
    {
        struct Pair { int a, b; int64_t d[4]; const char* what; };
        const Pair pairs[] = {{P_iabc, P_aibc, {o, v, v, v}, "V_iabc[i,a,b,c] - V_aibc[a,i,c,b]"},
                              {P_ijak, P_ijka, {o, o, v, o}, "V_ijak[i,j,a,k] - V_ijka[j,i,k,a]"},
                              {P_abic, P_abci, {v, v, o, v}, "V_abic[a,b,i,c] - V_abci[b,a,c,i]"},
                              {P_aijk, P_iajk, {v, o, o, o}, "V_aijk[a,i,j,k] - V_iajk[i,a,k,j]"},
                              {P_ijab, P_ijab, {o, o, v, v}, "V_ijab[i,j,a,b] - V_ijab[j,i,b,a]"}};
        for (const Pair& pr : pairs) {
            if (pr.a == P_ijab && !lam1) continue;
            double r[2];
            dev::exchange_asymmetry(V_[pr.a], V_[pr.b], pr.d, r, stream);
            if (!(r[0] <= 1e-10 * r[1])) {
                char buf[400];
                snprintf(buf, sizeof buf, "%s needs integrals with V_pqrs = V_qpsr: max |%s| = %.3e against max |V| = %.3e", who,
                         pr.what, r[0], r[1]);
                throw Error(buf);
            }
        }
    }
    if (t_end == t_begin) return 0.0;
    DevBufs bufs;
    // right amplitudes: T2o[x][y][f][z] = T[z,f,x,y], T2h[m][k][b][c] = T[b,c,m,k], as in ccsd_t
    double* T2o = bufs.get(o * o * v2);
    double* T2h = bufs.get(o * o * v2);
    const TView Tv = make_view(t2, {v, v, o, o});
    permute(1.0, Tv, "zfxy", 0.0, make_view(T2o, {o, o, v, v}), "xyfz");
    permute(1.0, Tv, "bcmk", 0.0, make_view(T2h, {o, o, v, v}), "mkbc");
    // left amplitudes in the same two layouts: L[a,b,i,j] = (2 lam2[a,b,i,j] + lam2[b,a,i,j]) / 3, l1 = lam1 / 2
    double* L2o = bufs.get(o * o * v2);
    double* L2h = bufs.get(o * o * v2);
    const TView Lv = make_view(lam2, {v, v, o, o});
    permute(2.0 / 3.0, Lv, "zfxy", 0.0, make_view(L2o, {o, o, v, v}), "xyfz");
    permute(1.0 / 3.0, Lv, "fzxy", 1.0, make_view(L2o, {o, o, v, v}), "xyfz");
    permute(2.0 / 3.0, Lv, "bcmk", 0.0, make_view(L2h, {o, o, v, v}), "mkbc");
    permute(1.0 / 3.0, Lv, "cbmk", 1.0, make_view(L2h, {o, o, v, v}), "mkbc");
    double* l1 = nullptr;
    if (lam1) {
        l1 = bufs.get(v * o);
        permute(0.5, make_view(lam1, {v, o}), "ai", 0.0, make_view(l1, {v, o}), "ai");
    }
    // the excitation-type blocks in the layouts of the de-excitation-type ones, so that the right triples are the products of
    // the left ones (and of ccsd_t), stride for stride: R1[i,f,a,b] = V_abic[a,b,i,f], R1s[f,i,a,b] = V_abic[b,a,i,f],
    // R2[i,j,a,m] = V_aijk[a,m,i,j].  Two o v^3 copies per call (3.2 GB each at (50,200)), released on return.
    double* R1 = bufs.get(o * v3);
    double* R1s = bufs.get(o * v3);
    double* R2 = bufs.get(o * o * o * v);
    permute(1.0, block(P_abic), "abif", 0.0, make_view(R1, {o, v, v, v}), "ifab");
    permute(1.0, block(P_abic), "baif", 0.0, make_view(R1s, {v, o, v, v}), "fiab");
    permute(1.0, block(P_aijk), "amij", 0.0, make_view(R2, {o, o, v, o}), "ijam");
    double* eps = bufs.get(n);
    dev::memcpy_h2d(eps, eps_host, sizeof(double) * n, stream);
    double* out = per_triple ? per_triple : bufs.get(t_end - t_begin);
    // batch: WR and WL of that many triples are held, so the default is half of ccsd_t's for the same 128 MB; each array
    // is built by products of its own triple alone (the per-triple values do not depend on the batch)
    int64_t batch = 0;
    if (const char* e = getenv("PYMES_TRIPLES_BATCH")) batch = atoll(e);
    if (batch <= 0) {
        const double budget = std::min(128.0 * (1 << 20), 0.25 * (double)dev::mem_free_bytes());
        batch = std::max<int64_t>(1, (int64_t)(budget / (16.0 * (double)v3)));
    }
    batch = std::min<int64_t>({batch, t_end - t_begin, 65535});
    double* WR = bufs.get(batch * v3);
    double* WL = bufs.get(batch * v3);
    double* partial = bufs.get(dev::triples_partial_doubles(nv, batch));
    const TriplesOperands right{R1, R1s, R2, T2o, T2h};
    const TriplesOperands left{V_[P_iabc], V_[P_aibc], V_[P_ijak], L2o, L2h};
    for (int64_t t0 = t_begin; t0 < t_end; t0 += batch) {
        const int64_t nt = std::min(batch, t_end - t0);
        for (int64_t q = 0; q < nt; ++q) {
            int i, j, k;
            unrank_triple(t0 + q, i, j, k);
            triples_W(*this, WR + q * v3, i, j, k, right);
            triples_W(*this, WL + q * v3, i, j, k, left);
        }
        dev::lambda_triples_energy(WR, WL, nt, t0, l1 ? V_[P_ijab] : nullptr, l1, eps, partial, out + (t0 - t_begin), no, nv,
                                   stream);
    }
    // the sum over the range in a fixed order (the same whatever the batch)
    std::vector<double> h(t_end - t_begin);
    dev::memcpy_d2h(h.data(), out, sizeof(double) * h.size(), stream);
    dev::stream_sync(stream);
    double e = 0.0;
    for (double x : h) e += x;
    return e;
}

// ---- frozen natural orbitals (include/pymes_amd.h, pymes_fno_density / pymes_derive_context) --------------------------------
namespace {
const char* kFnoHermitian = "frozen natural orbitals are built here for Hermitian integrals only, not for transcorrelated ones";
}

double Engine::fno_density(const double* Vijab, int n_frozen, double* D_host) {
    if (capturing_) throw Error("pymes_fno_density reads its result back: not inside a launch graph");
    if (!D_host) throw Error("pymes_fno_density: null pointer: D");
    if (n_frozen < 0 || n_frozen >= no)
        throw Error("pymes_fno_density: n_frozen = " + std::to_string(n_frozen) + " outside [0, no) = [0, " + std::to_string(no) +
                    ")");
    need_eps("pymes_fno_density");
    const int64_t o = no, v = nv;
    if (!Vijab) {
        if (!V_[P_ijab]) throw Error("pymes_fno_density needs the undressed integral block 'ijab', which has not been set");
        check_hermitian("pymes_fno_density", kFnoHermitian);
        Vijab = V_[P_ijab];
    }
    // the kernel reads t[c,a,i,j] as V[j,i,a,c] / d: V_ijab = V_jiba is required
    {
        const int64_t d[4] = {o, o, v, v};
        double r[2];
        dev::exchange_asymmetry(Vijab, Vijab, d, r, stream);
        if (!(r[0] <= 1e-10 * r[1])) {
            char buf[200];
            snprintf(buf, sizeof buf, "pymes_fno_density needs V_ijab = V_jiba: max |V_ijab - V_jiba| = %.3e against max |V| = %.3e",
                     r[0], r[1]);
            throw Error(buf);
        }
    }
    DevBufs bufs;
    double* partial = bufs.get(dev::fno_density_partial_doubles(no - n_frozen, nv));
    double* Dd = bufs.get(v * v);
    double* ed = bufs.get(1);
    dev::fno_density(Vijab, eps_o, eps_v, no, n_frozen, nv, partial, Dd, ed, stream);
    double e = 0.0;
    dev::memcpy_d2h(D_host, Dd, sizeof(double) * v * v, stream);
    dev::memcpy_d2h(&e, ed, sizeof(double), stream);
    dev::stream_sync(stream);
    return e;
}

void Engine::derive_from(Engine& src, int n_frozen, const double* C_host, int nv_dst) {
    const char* who = "pymes_derive_context";
    auto fail = [&](const std::string& m) { throw Error(std::string(who) + ": " + m); };
    if (&src == this) fail("the source and the destination are the same context");
    if (capturing_ || src.capturing_) fail("not inside a launch graph");
    if (src.shard_on_) fail("the source context shards its integrals (pymes_set_integral_shard): derive from a replicated context");
    if (shard_on_) fail("the destination context shards its integrals (pymes_set_integral_shard): it must be a plain empty context");
    if (src.direct_.on)
        fail("the source context is factor-direct (pymes_set_integral_direct) and holds no V_abcd: derive from a stored context");
    if (direct_.on) fail("the destination context is factor-direct (pymes_set_integral_direct): it must be a plain empty context");
    if (src.device != device) fail("the source and the destination are on different devices");
    if (!C_host) fail("null pointer: C");
    if (n_frozen < 0 || n_frozen >= src.no)
        fail("n_frozen = " + std::to_string(n_frozen) + " outside [0, no) = [0, " + std::to_string(src.no) + ")");
    if (nv_dst < 1 || nv_dst > src.nv)
        fail("nv_dst = " + std::to_string(nv_dst) + " outside [1, nv] = [1, " + std::to_string(src.nv) + "]");
    if (no != src.no - n_frozen || nv != nv_dst)
        fail("the destination context is (no, nv) = (" + std::to_string(no) + ", " + std::to_string(nv) + "), expected (" +
             std::to_string(src.no - n_frozen) + ", " + std::to_string(nv_dst) + ")");
    for (int pat = 0; pat < 16; ++pat) {
        if (!src.V_[pat]) fail("the source context lacks the integral block '" + canonical_name(pat) + "'");
        if (V_[pat] || Vd_[pat]) fail("the destination context is not empty (block '" + canonical_name(pat) + "' is set)");
    }
    src.check_hermitian(who, kFnoHermitian);
    dev::stream_sync(src.stream);
    const int64_t o0 = src.no, v0 = src.nv, o1 = no, v1 = nv;
    // ping-pong intermediates: the k-th transform of a block with m virtual indices holds o1^(4-m) v0^(m-k-1) v1^(k+1)
    // doubles; even k go to buffer A, odd k to B, the last one straight into the destination block (at most one v0^3 v1
    // intermediate: A of V_abcd after its first transform)
    int64_t needA = 1, needB = 1;
    for (int pat = 0; pat < 16; ++pat) {
        const int m = __builtin_popcount(pat);
        for (int k = 0; k + 1 < m; ++k) {
            int64_t sz = 1;
            for (int q = 0; q < 4 - m; ++q) sz *= o1;
            for (int q = 0; q < m - k - 1; ++q) sz *= v0;
            for (int q = 0; q < k + 1; ++q) sz *= v1;
            (k % 2 ? needB : needA) = std::max(k % 2 ? needB : needA, sz);
        }
    }
    DevBufs bufs;
    double* Cd = bufs.get(v0 * v1);
    dev::memcpy_h2d(Cd, C_host, sizeof(double) * v0 * v1, stream);
    double* A = bufs.get(needA);
    double* B = bufs.get(needB);
    const TView Cv = make_view(Cd, {v0, v1});
    const char* lab = "pqrs";
    for (int pat = 0; pat < 16; ++pat) {
        TView cur = src.block_view(src.V_[pat], pat);
        std::vector<int> vpos;
        for (int q = 0; q < 4; ++q) {
            if (pat >> (3 - q) & 1) vpos.push_back(q);
            else cur = slice(cur, q, n_frozen, o0);
        }
        const TView dst = block_view(ensure_block(pat), pat);
        if (vpos.empty()) {
            copy(cur, dst);
            continue;
        }
        for (size_t k = 0; k < vpos.size(); ++k) {
            const int q = vpos[k];
            // out[.., z, ..] = sum_x in[.., x, ..] C[x, z] at position q; the labels in front of q are GEMM batches
            int64_t dims[4];
            for (int r = 0; r < 4; ++r) dims[r] = cur.dim[r];
            dims[q] = v1;
            const bool last = k + 1 == vpos.size();
            const TView out = last ? dst : make_view(k % 2 ? B : A, 4, dims, nullptr);
            std::string lo = lab, lc = std::string(1, lab[q]) + "z", batch(lab, lab + q);
            lo[q] = 'z';
            contract(1.0, cur, lab, Cv, lc.c_str(), 0.0, out, lo.c_str(), batch.c_str());
            cur = out;
        }
    }
    dev::stream_sync(stream);
}

}  // namespace pymes
