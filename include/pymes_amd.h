/* pymes_amd — C-ABI of the MI355X-native CCSD/DCSD amplitude-update engine.
 *
 * This is the drop-in boundary for the hot path of nickirk/pymes (reference @
 * 2024_10_08).  The reference has no FFI: its seam is the module-level `einsum`
 * callable (pymes/solver/ccsd.py:11, mp2.py:5; historically `ctf.einsum`,
 * pymes/__init__.py:3) and the solver-class methods built on it.  Each entry point
 * below names the reference function it replaces.  pymes_amd/_lib.py binds exactly
 * these symbols with ctypes; INTEGRATION.md shows the reference-side stub.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; pymes_last_error()
 *     then returns a thread-local message.  No exception crosses the boundary.
 *   - all tensors are fp64, C-contiguous unless explicit strides (in elements) are
 *     given; "dev" pointers are device (HBM) addresses, "host" pointers host memory.
 *   - shapes follow the reference: T2 is [a,b,i,j] = (nv,nv,no,no), T1 is [a,i],
 *     Fock is [n,n], V[p,q,r,s] = <pq|rs>, block names are partition.py's
 *     (i,j,k,l occupied; a,b,c,d virtual).
 *   - one context per host thread; all work of a context is ordered on one HIP stream.
 */
#ifndef PYMES_AMD_H
#define PYMES_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pymes_ctx pymes_ctx;

/* ---- limits on nocc.  Three kernel families stage occupied-index tiles in the 64 KB of LDS a workgroup is given, and each has
 * its own largest nocc; everything else has none.
 *   PYMES_NOCC_MAX_FUSED   the fused pair kernels (one nocc x (nocc + 1) tile of doubles: pymes_pair_layouts[_sym],
 *                          pymes_symmetrised_assemble, the pair-sharded tail, the read-once amplitude tail): 90 x 91 x 8 = 65 520 B.
 *                          pymes_pairs_supported / pymes_sym_tail answer 0 above it; the residual and the right EOM sigma then
 *                          run their unfused forms (same results), the entry points named here and pymes_eom_sigma_apply_left
 *                          refuse.
 *   PYMES_NOCC_MAX_LAMBDA  the left assembly (that tile + 256 partial sums: pymes_eom_sigma_apply_left, pymes_lambda_step and the
 *                          solvers on them): 88 x 89 x 8 + 2048 = 64 704 B.  Refused above it before anything is allocated.
 *   PYMES_NOCC_MAX_BRA_DRESS  pymes_ladder_dress (the instantiated MFMA step counts); the CCSD step falls back to its Q_kb form. */
#define PYMES_NOCC_MAX_FUSED 90
#define PYMES_NOCC_MAX_LAMBDA 88
#define PYMES_NOCC_MAX_BRA_DRESS 80

/* ---- library / context ------------------------------------------------------- */
const char* pymes_last_error(void);
const char* pymes_backend(void);                 /* "hip-gfx950" for the product library */
int pymes_ctx_create(pymes_ctx** out, int device, int no, int nv, uint64_t workspace_bytes /* 0 = auto */);
int pymes_ctx_destroy(pymes_ctx* ctx);
/* A context runs on a HIP stream of its own; pymes_ctx_set_stream binds another one (after completing what was
 * enqueued on the old one) — e.g. torch's current stream, so that RCCL collectives and engine kernels are ordered on
 * the device without host fences (pymes_amd/dist.py). */
int pymes_ctx_set_stream(pymes_ctx* ctx, void* hip_stream);
int pymes_ctx_sync(pymes_ctx* ctx);
int pymes_ctx_workspace(pymes_ctx* ctx, uint64_t* capacity_bytes, uint64_t* high_water_bytes);

/* ---- device memory ------------------------------------------------------------ */
/* buffers belong to the context: pymes_ctx_destroy releases whatever has not been passed to pymes_free */
int pymes_malloc(pymes_ctx* ctx, uint64_t bytes, void** dev_ptr);
int pymes_free(pymes_ctx* ctx, void* dev_ptr);
int pymes_live_allocations(int64_t* n);          /* device allocations of this library not yet released (leak tests) */
int pymes_mem_info(pymes_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes);   /* hipMemGetInfo of the context's device */
/* Number of T1 dressings the context's dressed blocks have seen: every get_T1_dressed_V-shaped call (pymes_ccsd_dress_V,
 * _slab), every pymes_ccsd_residuals / _iterate / _sharded_residuals with T1 != 0 and every replay of a recorded graph that
 * contains one.  A holder of dressed blocks (ccsd.py:290-421 hands out a dictionary; here the blocks stay in the context)
 * remembers the value and refuses to read blocks that have been dressed again since. */
int pymes_dress_generation(pymes_ctx* ctx, uint64_t* n);

/* ---- phase launches.  The small kernels between two big products (a (20,80) iteration has ~60 of 5-35 us) are not launched
 * one by one: inside the library they are recorded with the address ranges they read and write and launched level by level of
 * their dependency graph, ONE grid per level carrying the blocks of all its tasks (a dependent launch costs 1.9 us on
 * this chip, so the seams stay kernel boundaries and what goes is the serialisation of INDEPENDENT kernels).  Every entry point
 * of this header leaves nothing recorded behind when it returns; results are the same as with immediate launches.
 * pymes_phase_enable: 1 on, 0 off, -1 as the environment says (PYMES_PHASE=0 off, =serial one task per level; default on) — per
 * calling thread.  pymes_phase_stats: tasks recorded / grids launched / levels / flushes by the calling thread so far. */
int pymes_phase_enable(int mode);
/* pymes_phase_hold(1): the calls that follow leave their small operations recorded instead of launching them when they return,
 * so that operations of SEVERAL calls share levels (an iteration's two amplitude updates, pymes_cc_update_to, and the overlaps
 * of its mixer); pymes_phase_hold(0) launches them.  Anything that synchronises or copies launches them first, held or not. */
int pymes_phase_hold(int on);
int pymes_phase_stats(int64_t* tasks, int64_t* launches, int64_t* levels, int64_t* flushes);

/* ---- launch graphs (hipGraph): the loop body of a small, launch-bound solve is recorded once and replayed.
 * Between begin and end the context's entry points only RECORD their kernels (nothing executes, nothing may
 * synchronise: no pymes_dots / pymes_download / pymes_free); every pointer passed in is baked into the graph, so the
 * replayed segment must work on fixed buffers (pymes_amd/solver/ccsd.py keeps T1/T2 and the residuals in place).
 * The reference has no counterpart: its loop body (ccsd.py:159-209) is re-interpreted by Python every iteration. */
int pymes_graph_begin(pymes_ctx* ctx);
int pymes_graph_end(pymes_ctx* ctx, void** graph);
int pymes_graph_abort(pymes_ctx* ctx);
int pymes_graph_launch(pymes_ctx* ctx, void* graph);
int pymes_graph_destroy(pymes_ctx* ctx, void* graph);
int pymes_upload(pymes_ctx* ctx, void* dst_dev, const void* src_host, uint64_t bytes);   /* synchronous */
int pymes_download(pymes_ctx* ctx, void* dst_host, const void* src_dev, uint64_t bytes); /* synchronous */
int pymes_copy(pymes_ctx* ctx, void* dst_dev, const void* src_dev, uint64_t bytes);      /* stream-ordered */
int pymes_memset_zero(pymes_ctx* ctx, void* dst_dev, uint64_t bytes);

/* ---- generic tensor engine: the `einsum` seam (ccsd.py:11, mp2.py:5) ------------ */
/* C[lc] = alpha * sum_{contracted} A[la] * B[lb] + beta * C[lc]; one-letter labels; strides
 * may be NULL (contiguous); `batch` lists free labels to run as GEMM batches ("" = none).
 * Strides (here, in pymes_permute and in the device forms of pymes_set_V_pqrs / pymes_set_V_block; with on_device == 0 those
 * two read a C-contiguous host array and neither use nor check `strides`) count ELEMENTS and are zero or positive, of
 * tensors of rank 0..6:
 *  - an INPUT axis may have stride 0 (the operand is shared along it); an output has neither a zero stride nor two index
 *    tuples on one element;
 *  - a negative stride is refused with an error that names the argument (the product kernels read a pitch as an unsigned
 *    distance): pass a reversed copy;
 *  - no alignment is asked of a base pointer or a pitch beyond 8 bytes; the 16-byte loads are chosen only where both allow;
 *  - ONE-ELEMENT OVER-READ: a product may load the 8 bytes that follow the last element of A or B (the second half of a pair
 *    load past an odd contiguous extent; its value reaches no stored element of C).  That double must lie inside the same
 *    allocation: a view of an input must not end flush with the end of its allocation.  Nothing outside the view of C is
 *    written, and with beta == 0 nothing of C is read. */
int pymes_contract(pymes_ctx* ctx, double alpha,
                   const double* A_dev, const char* la, const int64_t* dimA, const int64_t* strideA,
                   const double* B_dev, const char* lb, const int64_t* dimB, const int64_t* strideB,
                   double beta, double* C_dev, const char* lc, const int64_t* dimC, const int64_t* strideC,
                   const char* batch);
/* out[lo] = alpha * in[li] + beta * out[lo]; `lo` is a permutation of `li` */
int pymes_permute(pymes_ctx* ctx, double alpha, const double* in_dev, const char* li, const int64_t* dim_in,
                  const int64_t* stride_in, double beta, double* out_dev, const char* lo,
                  const int64_t* stride_out);
/* raw fp64 MFMA GEMM (kernel-level tests): C(m,n) = alpha*sum_k A(m,k)B(k,n) + beta*C(m,n),
 * A(m,k) = A[m*a_sm + k*a_sk], B(k,n) = B[k*b_sk + n*b_sn], C(m,n) = C[m*ldc + n] */
int pymes_dgemm(pymes_ctx* ctx, int64_t M, int64_t N, int64_t K, double alpha, const double* A_dev, int64_t a_sm,
                int64_t a_sk, const double* B_dev, int64_t b_sk, int64_t b_sn, double beta, double* C_dev,
                int64_t ldc);
/* ... with the beta term read from another array of C's layout: C = alpha*A*B + beta*Cin (Cin_dev NULL: from C itself) */
int pymes_dgemm_cin(pymes_ctx* ctx, int64_t M, int64_t N, int64_t K, double alpha, const double* A_dev, int64_t a_sm,
                    int64_t a_sk, const double* B_dev, int64_t b_sk, int64_t b_sn, double beta, const double* Cin_dev,
                    double* C_dev, int64_t ldc);

/* ---- integrals: pymes/integral/partition.py:4-39 -------------------------------- */
/* V[n,n,n,n] (host: C-contiguous, strides ignored; device: element strides or NULL) -> 16 blocks */
int pymes_set_V_pqrs(pymes_ctx* ctx, const double* V, int on_device, const int64_t* strides);
/* a single block by its partition.py name ("abcd", "ijab", ...); n_elements must be the block's size for this
 * context (a mis-shaped block is refused instead of being read out of bounds) */
int pymes_set_V_block(pymes_ctx* ctx, const char* name, const double* data, int64_t n_elements, int on_device,
                      const int64_t* strides);
/* Electron-exchange symmetry V_pqrs = V_qpsr, which the symmetry-reduced residual (PYMES_SYM_LADDER / PYMES_SYM_RINGS)
 * presumes and the reference's own Ex += Ex^T (ccd.py:245-249) relies on: out = { max |V_pqrs - V_qpsr| over the blocks
 * that are set (infinity when a block's partner is absent), max |V| }.  pymes_exchange_asymmetry is the same test for
 * any pair A [d0,d1,d2,d3], B [d1,d0,d3,d2] on the device (T2 against itself: T_abij = T_baji). */
int pymes_V_exchange_asymmetry(pymes_ctx* ctx, double* out_host);
int pymes_exchange_asymmetry(pymes_ctx* ctx, const double* A_dev, const double* B_dev, const int64_t* dims,
                             double* out_host);
/* V[p,q,r,s] = sum_Q B[Q,p,r] B[Q,q,s]  (density-fitted / synthetic input), B_host is [naux,n,n] */
int pymes_set_V_from_factors(pymes_ctx* ctx, const double* B_host, int naux);
/* Integral sharding (opt-in; before any pymes_set_V_* call): the context never allocates V_abcd.  It stores instead the
 * undressed pair-packed rows [r0,r1) of rank `rank` of `world` (the chunk of v(v+1)/2 pair rows P(a,b), a >= b, that the
 * sharded residual steps give that rank): V^+ / V^- as dev ladder_pack_V writes them, row pitches ldp / ldm.  set_V_pqrs and
 * set_V_block("abcd") from the host upload only the rank's planes V[a,b,:,:] (one bounded staging buffer, 1 GiB);
 * set_V_from_factors forms the rows straight from B.  The other 15 blocks are held as ever.  Only the sharded ladders of that
 * (rank, world) are served; every entry point that needs the full or dressed V_abcd fails and names the mode (the block
 * pointer, set_V_block("abcd") from device memory, pymes_ladder, pymes_doubles_residual, pymes_ccsd_residuals /
 * _iterate, pymes_ccsd_dress_abcd_rows, dressed or other rows of pymes_ladder_sym, the EOM sigma). */
int pymes_set_integral_shard(pymes_ctx* ctx, int rank, int world);
/* Factor-direct particle ladder (opt-in; before any pymes_set_V_* call; not together with pymes_set_integral_shard): nothing of
 * size v^4 is ever allocated.  Only pymes_set_V_from_factors sets the integrals of such a context (set_V_pqrs / set_V_block
 * are refused: there are no factors): it forms the 15 other blocks as ever, keeps a compact device copy of the
 * virtual-virtual factors B_vv (zero-padded [nv][naux up to 8][nv up to 64]) and allocates one pair of chunk buffers for V^+ /
 * V^- rows at the ladder pitches, within chunk_bytes (0: the environment's PYMES_DIRECT_CHUNK_BYTES, default 1 GiB; at least
 * one row).  The undressed pair-packed ladders (pymes_ladder_sym, the ladders inside pymes_ccsd_residuals / _iterate and the
 * symmetric pymes_doubles_residual) rebuild their rows from B_vv chunk by chunk in every call: npp v^2 naux 2 flops per call in
 * exchange for 8 v^4 (block) + 8 v^4 (packed rows) bytes.  The T1 dressing of the ladder rides on tau and the Q_kb products
 * (PYMES_LADDER_DRESS=1 is an error here).  PYMES_DIRECT_BUILDER=gemm|fused selects the row builder: batched products into
 * planes that dev ladder_pack_V packs (every backend), or one gfx950 kernel from B_vv straight into the rows (the default
 * where the backend has it).  Everything
 * that needs the full, dressed or stored V_abcd fails and names the mode: the block pointer, pymes_ladder, the general or
 * dressed pymes_doubles_residual, pymes_ccsd_dress_abcd_rows, dressing abcd, dressed pymes_ladder_sym, pymes_ladder_sym_multi
 * / _adjoint*, the EE / EA sigma, the EOM diagonals, pymes_rdm2_expectation, pymes_derive_context from or into it. */
int pymes_set_integral_direct(pymes_ctx* ctx, int64_t chunk_bytes);
/* info[5] = { naux, rows per chunk, bytes of B_vv, bytes of the chunk buffers, builder (0 gemm, 1 fused) } of such a context */
int pymes_direct_info(pymes_ctx* ctx, int64_t* info);
/* builds the rows [r0,r1) (at most one chunk) into the chunk buffers and returns them read-only (device pointers, row
 * pitches; valid until the next ladder call): for tests */
int pymes_direct_rows(pymes_ctx* ctx, int64_t r0, int64_t r1, const double** vp, const double** vm, int64_t* ldp, int64_t* ldm);
/* bytes the context holds for integrals: undressed and dressed blocks, the stored / packed V_abcd rows, the static packs */
int pymes_integral_bytes(pymes_ctx* ctx, int64_t* bytes);
/* read-only view of the stored rows of a sharded context: device pointers, the pair-row range and the row pitches */
int pymes_shard_rows_ptr(pymes_ctx* ctx, const double** vp, const double** vm, int64_t* row0, int64_t* row1, int64_t* ldp,
                         int64_t* ldm);
/* device address of a block ("dressed" = output of pymes_ccsd_dress_V); NULL+error if absent */
int pymes_V_block_ptr(pymes_ctx* ctx, const char* name, int dressed, double** dev_ptr, int64_t* n_elements);
/* diag(f): eps_o[no], eps_v[nv] used by the denominators (ccsd.py:149-156) */
int pymes_set_orbital_energies(pymes_ctx* ctx, const double* eps_o_host, const double* eps_v_host);

/* ---- (T): the perturbative triples correction of CCSD(T) (closed shell, canonical orbitals) -------------------------------
 * Notation V[p,q,r,s] = <pq|rs>, T[a,b,i,j], t1[a,i], eps = diag(f).  For an occupied triple (i,j,k):
 *   w_ijk[a,b,c] = sum_f V_iabc[i,f,a,b] T[c,f,k,j] - sum_m V_ijak[i,j,a,m] T[b,c,m,k]
 *   W_ijk[a,b,c] = w_ijk[abc] + w_ikj[acb] + w_jik[bac] + w_jki[bca] + w_kij[cab] + w_kji[cba]
 *   Y_ijk[a,b,c] = W_ijk[abc] + V_ijab[j,k,b,c] t1[a,i] + V_ijab[i,k,a,c] t1[b,j] + V_ijab[i,j,a,b] t1[c,k]
 *   R(Y)[a,b,c]  = 4Y[abc] + Y[bca] + Y[cab] - 2Y[cba] - 2Y[acb] - 2Y[bac]
 *   S_ijk        = 1/3 sum_abc W[abc] R(Y)[abc] / (eps_i + eps_j + eps_k - eps_a - eps_b - eps_c)
 *   E(T)         = sum_{i >= j >= k} m_ijk S_ijk,   m = 6 (i > j > k), 3 (two equal), 1 (i = j = k)
 * The unique triples are numbered i ascending, then j <= i, then k <= j (t = i(i+1)(i+2)/6 + j(j+1)/2 + k);
 * pymes_ccsd_t_triples gives their number o(o+1)(o+2)/6.  pymes_ccsd_t sums m_ijk S_ijk over [t_begin, t_end) (one rank's
 * share: the caller adds the ranks' sums) into *e_out_host and, if per_triple_dev is not NULL, writes the m_ijk S_ijk of the
 * range there (t_end - t_begin doubles, device).  eps_host [n] (host), t1_dev [v,o] (NULL: CCD amplitudes), t2_dev [v,v,o,o]
 * with T_abij = T_baji.  Reads only the UNDRESSED blocks iabc, aibc, ijak (and ijab with t1): valid after pymes_ccsd_dress_V and
 * on a context with pymes_set_integral_shard.  Refused: a missing block (named), a call while a launch graph is recorded,
 * integrals without V_pqrs = V_rspq (max |V_iabc - V_abic|, |V_ijak - V_aijk| above 1e-10 max |V|: transcorrelated
 * Hamiltonians).  Each per-triple value and the sum (fixed order) are the same whatever the batch of triples the call
 * holds at once (PYMES_TRIPLES_BATCH=<n> forces it).  Synchronises; frees what it allocates before it returns. */
int pymes_ccsd_t_triples(pymes_ctx* ctx, int64_t* n_triples);
int pymes_ccsd_t(pymes_ctx* ctx, const double* eps_host, const double* t1_dev, const double* t2_dev, int64_t t_begin,
                 int64_t t_end, double* per_triple_dev, double* e_out_host);

/* ---- Lambda-CCSD(T): the triples correction with Lambda as the left state (Kucharski-Bartlett, Taube-Bartlett) ---------------
 * The triples correction for Hamiltonians without V_pqrs = V_rspq (transcorrelated integrals), which pymes_ccsd_t refuses; for
 * Hermitian integrals the more robust one away from equilibrium.  Closed shell, canonical orbitals (the f_ov lam2 term of the
 * general formula vanishes), notation as above.  lam1 [v,o], lam2 [v,v,o,o] are the library's Lambda (pymes_lambda_step:
 * A^T lam + eta = 0, eta2 = 2 V_ijab - V_ijba, plain inner product), converted once per call:
 *   L[a,b,i,j] = (2 lam2[a,b,i,j] + lam2[b,a,i,j]) / 3        l1[a,i] = lam1[a,i] / 2
 * (in spin orbitals the doubles multiplier is 2L - L^x, the singles multiplier 2 l1).  For an occupied triple (i,j,k):
 *   wR_ijk[a,b,c] = sum_f V_abic[a,b,i,f] T[c,f,k,j] - sum_m V_aijk[a,m,i,j] T[b,c,m,k]      (right: targets in the bra)
 *   wL_ijk[a,b,c] = sum_f V_iabc[i,f,a,b] L[c,f,k,j] - sum_m V_ijak[i,j,a,m] L[b,c,m,k]      (left: w above, L for T)
 *   WR, WL        = the six-permutation sums of wR, wL, as W_ijk above
 *   YL[a,b,c]     = WL[abc] + V_ijab[j,k,b,c] l1[a,i] + V_ijab[i,k,a,c] l1[b,j] + V_ijab[i,j,a,b] l1[c,k]
 *   S_ijk         = 1/3 sum_abc WR[abc] R(YL)[abc] / (eps_i + eps_j + eps_k - eps_a - eps_b - eps_c)
 *   E_Lambda(T)   = sum_{i >= j >= k} m_ijk S_ijk
 * t1 does not enter (the right triples are connected); lam1_dev may be NULL (CCD, electron gas).  The formula needs
 * V_pqrs = V_qpsr, T_abij = T_baji and the same symmetry of lam2, nothing else.  Triple numbering, ranges, per_triple_dev and
 * e_out_host as for pymes_ccsd_t.  Reads only the UNDRESSED blocks iabc, aibc, ijak, abic, aijk (ijab with lam1) and, for the
 * symmetry check, their partners ijka, abci, iajk: valid after pymes_ccsd_dress_V and on a context with
 * pymes_set_integral_shard (no V_abcd).  Refused: a missing block (named), a call while a launch graph is recorded, integrals
 * without V_pqrs = V_qpsr on those blocks (above 1e-10 max |V|; the block pair is named).  There is no Hermiticity check.  WR
 * and WL are each the twelve products of pymes_ccsd_t (the excitation-type blocks are copied once per call into the layouts
 * of the de-excitation-type ones: two o v^3 arrays); both are held per batch, so the default batch is half of pymes_ccsd_t's
 * (PYMES_TRIPLES_BATCH=<n> forces it).  Each per-triple value and the sum (fixed order) are the same whatever the batch.
 * Synchronises; frees what it allocates before it returns. */
int pymes_ccsd_t_lambda(pymes_ctx* ctx, const double* eps_host, const double* t2_dev, const double* lam1_dev,
                        const double* lam2_dev, int64_t t_begin, int64_t t_end, double* per_triple_dev, double* e_out_host);

/* ---- frozen natural orbitals (FNO) and frozen core (closed shell, canonical orbitals, Hermitian integrals) -----------------
 * Orbital window: the n_frozen lowest occupied orbitals are dropped, the active ones are [n_frozen, no), no' = no - n_frozen.
 * Amplitudes over the active occupied orbitals and all virtuals, eps = the context's orbital energies (pymes_set_orbital_energies):
 *   t[a,b,i,j] = V_ijab[i,j,a,b] / (eps_i + eps_j - eps_a - eps_b),      E_MP2 = sum (2 t[a,b,i,j] - t[b,a,i,j]) V_ijab[i,j,a,b]
 * and the spin-summed virtual block of the unrelaxed MP2 density (symmetric; eigenvalues = natural occupations in [0, 2]):
 *   D[a,b] = 2 sum_{c,i,j} (2 t[a,c,i,j] - t[c,a,i,j]) t[b,c,i,j]
 * pymes_fno_density writes D [nv,nv] (host, row-major) and E_MP2 of the window.  v_ijab_dev: a device [no,no,nv,nv] V_ijab
 * (e.g. formed from density-fitting factors), NULL = the context's own undressed 'ijab' block (then the integrals must be
 * Hermitian, checked as by pymes_ccsd_t).  The amplitudes are formed on the fly (no o^2 v^2 array); the kernel reads
 * t[c,a,i,j] as V_jiac / d, so V_ijab = V_jiba is checked.  Fixed summation order without atomics: two calls give bit-identical
 * D and E_MP2.  Refused: n_frozen outside [0, no), missing orbital energies or blocks, non-Hermitian (transcorrelated)
 * integrals, a V_ijab without the exchange symmetry, a call while a launch graph is recorded.
 * pymes_derive_context fills the EMPTY context dst, created with (no - n_frozen, nv_dst), with all 16 blocks of the space
 * whose occupied orbitals are [n_frozen, no) of src and whose virtuals are the columns of C (host, row-major [nv, nv_dst]):
 *   V'[p',q',r',s'] = V[p,q,r,s] with occupied indices sliced (p = p' + n_frozen) and every virtual index x' = sum_x C[x,x'] x
 * One quarter-transform (fp64 MFMA GEMM) per virtual index, through at most one nv^3 nv_dst intermediate; nothing passes through
 * the host.  dst then serves every call of a context (ladder packs, T1 dressing, pymes_ccsd_t); its orbital energies are the
 * caller's to set.  Refused: src == dst, a sharded src or dst (pymes_set_integral_shard), a src without all 16 blocks or
 * with non-Hermitian integrals, a dst with any block set or of the wrong size, n_frozen outside [0, no), nv_dst outside
 * [1, nv], different devices, a recorded launch graph.  Both calls synchronise and free what they allocate. */
int pymes_fno_density(pymes_ctx* ctx, const double* v_ijab_dev, int n_frozen, double* D_host, double* e_mp2_host);
int pymes_derive_context(pymes_ctx* src, pymes_ctx* dst, int n_frozen, const double* C_host, int nv_dst);

/* ---- the CC hot path ------------------------------------------------------------- */
/* pymes/solver/mp2.py:9-22: T2 = V_abij/(D+shift) into t2_dev; e_out = {direct, exchange} */
int pymes_mp2(pymes_ctx* ctx, double level_shift, double* t2_dev, double* e_out_host);
/* CCSD.get_T1_dressed_fock, ccsd.py:226-288 (f and fd are [n,n] on the device) */
int pymes_ccsd_dress_fock(pymes_ctx* ctx, const double* f_dev, const double* t1_dev, double* fd_dev);
/* CCSD.get_T1_dressed_V, ccsd.py:290-421; block_mask bit p = pattern id of the block
 * (bit 3-pos set when index `pos` is virtual: "abcd"=15, "klij"=0, "ijab"=3, "abij"=12 ...).
 * PYMES_DRESS_ABIJ_REDUCED: V~_abij without its V_pqcd t_ci t_dj and t_ak t_bl V~_klrs terms, i.e. what is left of
 * it once those terms travel with the ladders (the amplitude-side mode of pymes_residual_finish forms the same
 * quantity implicitly; the explicit block is kept for inspection and tests). */
#define PYMES_DRESS_ABIJ_REDUCED (1u << 16)
int pymes_ccsd_dress_V(pymes_ctx* ctx, const double* t1_dev, uint32_t block_mask);
/* the same for the range [p_begin,p_end) of the FIRST and [q_begin,q_end) of the SECOND index only (an empty range =
 * the whole index; a block in which the restricted index is occupied is dressed as a whole, so "klij" may ride in the same
 * call and share its V_klcd t_dj intermediate with "iabj"): "iajb" / "iabj" with a q-range is what
 * one rank's column slab of pymes_residual_slab reads, "abij" with (p,q) = (rows a of the rank's pairs, b below their
 * end) and the transposed pair of ranges is what the pair-sharded tail reads — no exchange */
int pymes_ccsd_dress_V_slab(pymes_ctx* ctx, const double* t1_dev, uint32_t block_mask, int p_begin, int p_end,
                            int q_begin, int q_end);
/* CCSD.get_singles_residual, ccsd.py:423-438 */
int pymes_ccsd_singles_residual(pymes_ctx* ctx, const double* fd_dev, const double* t1_dev, const double* t2_dev,
                                double* r1_dev);
/* The same residual as a partial sum over rank `rank`'s chunk of the occupied summation index (one process per GPU; needs
 * T_abij = T_baji): the caller all-reduces the [nv][no] results (f~_ai enters on rank 0).  world = 1 is the whole residual. */
int pymes_ccsd_singles_residual_partial(pymes_ctx* ctx, const double* fd_dev, const double* t1_dev, const double* t2_dev,
                                        double* r1_dev, int rank, int world, uint32_t flags /* PYMES_REUSE_LAYOUTS or 0 */);
/* CCD.get_residual, ccd.py:164-254 (and CCSD.get_doubles_residual, ccsd.py:440-456, with
 * PYMES_USE_DRESSED).  flags: */
#define PYMES_DCD 1u          /* is_dcd / is_dcsd */
#define PYMES_USE_DRESSED 2u  /* read the T1-dressed blocks instead of the undressed ones */
#define PYMES_SKIP_LADDER 4u  /* leave out V_abcd.T (ccd.py:187) — it is added per slab by pymes_ladder[_sym] */
#define PYMES_SYM_LADDER 8u   /* evaluate V_abcd.T in pair-packed form (1/4 of the flops); requires
                                 V_abcd = V_badc and T_cdij = T_dcji, true for every closed-shell solve that
                                 starts from MP2 or from symmetric amplitudes */
#define PYMES_SLAB_RINGS_ONLY 64u   /* pymes_residual_slab: only the ring products (rows of ETd / ETx) ... */
#define PYMES_SLAB_LADDERS_ONLY 128u /* ... only the ladders (rows of L, Q_kb).  One process per GPU calls the two halves
                                 separately: the all-gathers of ETd / ETx are started after the first and fly while the
                                 second — whose output stays on the rank — is computed */
#define PYMES_REUSE_LAYOUTS 32u /* the caller's promise that t2 has not changed since the preceding pymes_residual_slab call
                                 on it: its pair layouts (Td, Tx, 2T - T^(ab)) are read again instead of being rebuilt
                                 (pymes_residual_finish, pymes_ccsd_singles_residual_partial) */
#define PYMES_T1_ZERO (1u << 20) /* pymes_ccsd_residuals / _iterate: the caller knows that t1 == 0 exactly (the MP2 start; every
                                  * pass of a momentum-conserving system): the residuals come from the undressed f and V */
#define PYMES_SYM_RINGS 16u   /* same precondition: merge the o^3v^3 ring/exchange products through the symmetry of
                                 the pair matrices (C / D form: 4 products instead of 10; 3 instead of 5 for DCSD) */
int pymes_doubles_residual(pymes_ctx* ctx, const double* f_dev, const double* t2_dev, double* r2_dev,
                           uint32_t flags);
/* the particle-particle ladder on an a-slab (ccd.py:187): R[a0:a1] = beta*R[a0:a1] + V_abcd[a0:a1].T */
int pymes_ladder(pymes_ctx* ctx, const double* t2_dev, double* r2_dev, int a_begin, int a_end, int dressed,
                 double beta);
/* pair-packed form of the same term.  L is [v(v+1)/2][o*o] on the device; row r = P(a,b) = a(a+1)/2+b
 * (a >= b) holds [ LS (o(o+1)/2 entries, P(i,j)) | LA (o(o-1)/2 entries, Q(i,j) = i(i-1)/2+j) ].
 * pymes_ladder_sym fills rows [row_begin,row_end) (the shardable unit); pymes_ladder_sym_unpack adds
 * R[a,b,i,j] = beta R + LS + sgn(a-b) sgn(i-j) LA from a complete L.
 * hole_ladder: 0 = ccd.py:187 only; 1 / 2 = also add the hole ladder sum_kl I_klij T_abkl (ccd.py:175-186) to the
 * same rows, evaluated pair-packed as well (I_klij = I_lkji), with I = V_klij + V_klcd T_cdij (1, CCD/CCSD) or
 * I = V_klij (2, DCD/DCSD). */
int pymes_ladder_sym(pymes_ctx* ctx, const double* t2_dev, double* L_dev, int64_t row_begin, int64_t row_end,
                     int dressed, int hole_ladder);
int pymes_ladder_sym_unpack(pymes_ctx* ctx, const double* L_dev, double* r2_dev, double beta);
/* The particle ladder of pymes_ladder_sym (all rows, no hole ladder) for k exchange-symmetric vectors at once:
 * x_dev[z] are k device arrays [v,v,o,o], L_all_dev k consecutive arrays [v(v+1)/2][o*o].  One batched GEMM launch per half
 * over all vectors — the sigma builds of every vector of an EOM-CCSD Davidson pass (eom_ccsd.py:95-101, :383). */
int pymes_ladder_sym_multi(pymes_ctx* ctx, const double* const* x_dev, int k, double* L_all_dev, int dressed);
/* T1 dressing of the bra of the pair-packed V_abcd (ccsd.py:414-419, as far as the pair-packed ladder reads it):
 * V_dev, W_dev [r1 - r0][ld] hold the rows P(a,b) = a(a+1)/2 + b in [r0,r1) of one half of the packed block (columns (c,d)
 * packed, pitch ld = a multiple of 16 doubles), Pk_dev [v*o][ld] the rows x*o + k of V_kxcd packed the same way (x slow), t1_dev [v,o]:
 *   W[P(a,b)] = V[P(a,b)] - sum_k t1[a,k] Pk[(b,k)] -+ sum_k t1[b,k] Pk[(a,k)]
 * ("-" for the symmetric half V_abcd + V_abdc, "+" with minus_half = 1 for V_abcd - V_abdc, whose rows a == b stay zero).
 * nocc <= PYMES_NOCC_MAX_BRA_DRESS; the packed rows of 16 consecutive a within 2 GB (nvirt up to ~320). */
int pymes_ladder_dress(pymes_ctx* ctx, const double* V_dev, const double* Pk_dev, const double* t1_dev, double* W_dev,
                       int64_t ld, int64_t r0, int64_t r1, int minus_half);
/* The three pair layouts of an amplitude-like array X [v,v,o,o] in one pass: Xd[(a,i),(b,j)] = X_abij,
 * Xx[(a,j),(b,i)] = X_abij, Xt[(a,i),(b,j)] = 2 X_abij - X_baij (each [o*v][o*v]; Xd_dev may be NULL).  ccd.py:199 /
 * eom_ccsd.py:352-373 form these index orders implicitly inside their einsum calls. */
int pymes_pair_layouts(pymes_ctx* ctx, const double* x_dev, double* Xd_dev, double* Xx_dev, double* Xt_dev);
/* P(ijab,jiba) symmetrisation and assembly in one pass (ccd.py:249-252, eom_ccsd.py:377):
 *   R_abij = V_abij + unpack(L)_abij + N_abij + N_baji + D[(a,i),(b,j)] + D[(b,j),(a,i)] + X[(a,j),(b,i)] + X[(b,i),(a,j)]
 * with V [v,v,o,o] (NULL: 0; may be R), L the pair-packed rows of pymes_ladder_sym (NULL: none), N [v,v,o,o], D and X
 * [o*v][o*v] pair matrices ((a,i) = a*o + i).  Needs o(o+1) doubles of LDS (pymes_residual_finish uses it internally). */
int pymes_symmetrised_assemble(pymes_ctx* ctx, const double* V_dev, const double* L_dev, const double* N_dev,
                               const double* D_dev, const double* X_dev, double* R_dev);
/* Rows [row_begin,row_end) of L += pair-packed sum_kl I_klij X_abkl for a caller-supplied I [o,o,o,o] with I_klij = I_lkji
 * and X [v,v,o,o] with X_abkl = X_balk: the hole-ladder-shaped terms of the EOM-CCSD sigma, eom_ccsd.py:380-382
 * (u2 against V_klij + V_klcd T_cdij; T against V_kldc u2_dcij), at 1/4 of the flops of the plain product.  y_dev
 * (optional, [v,v,o,o], y_cdij = y_dcji): sum_cd V_klcd y_cdij is added to I on the way, formed pair-packed as well (the
 * caller then passes only the y-independent part of I). */
int pymes_hole_ladder_packed(pymes_ctx* ctx, const double* x_dev, const double* I_dev, double* L_dev, int64_t row_begin,
                             int64_t row_end, const double* y_dev);
/* pymes_hole_ladder_packed (all rows) for k vectors in batched launches: L_all_dev[z] += rows(x_dev[z]) . (2 I_dev[z]
 * [+ 2 V_klcd y_dev[z]_cdij]); entries of x_dev (or of I_dev) may all be the same array, which is then packed once —
 * eom_ccsd.py:380-382 over the vectors of a Davidson pass.  y_dev may be NULL. */
int pymes_hole_ladder_packed_multi(pymes_ctx* ctx, const double* const* x_dev, const double* const* I_dev,
                                   const double* const* y_dev, int k, double* L_all_dev);
/* ---- whole steps of the CCSD / DCSD loop body (ccsd_residuals, ccsd_iterate) ---------------------------------------
 * pymes_ccsd_residuals: ccsd.py:161-171 in ONE call — T1-dressed Fock matrix (:163), the dressed blocks the loop reads (:165),
 * R1 [v,o] (:167) and R2 [v,v,o,o] (:171) from f [n,n], t1 [v,o], t2 [v,v,o,o] (all on the device).  The symmetry-reduced
 * form on one rank: needs V_pqrs = V_qpsr (pymes_V_exchange_asymmetry) and T_abij = T_baji (pymes_exchange_asymmetry) — the
 * caller's promise; anything else goes through pymes_ccsd_doubles_residual.  Only enqueues kernels, on buffers the context
 * holds from the first call to pymes_ccsd_release (replayable as a launch graph between those two).
 * pymes_ccsd_iterate: one fixed-point pass without a mixer (ccsd.py:159-197 with is_diis = False): residuals, dT = R / (D +
 * level_shift) (pymes_set_orbital_energies first), T += delta dT in place, energies and norms of the updated amplitudes:
 * out6 = {one-body, direct, exchange, |t2|^2, |dt2|^2, |t1|^2} (host).  With a mixer: pymes_ccsd_residuals,
 * pymes_cc_update_to, pymes_diis_mix, pymes_energy_norms — the sequence of pymes_amd/solver/ccsd.py. */
int pymes_ccsd_residuals(pymes_ctx* ctx, const double* f_dev, const double* t1_dev, const double* t2_dev, uint32_t flags,
                         double* r1_dev, double* r2_dev);
int pymes_ccsd_iterate(pymes_ctx* ctx, const double* f_dev, double* t1_dev, double* t2_dev, uint32_t flags, double level_shift,
                       double delta, double* dt1_dev, double* dt2_dev, double* out6_host);
int pymes_ccsd_release(pymes_ctx* ctx);

/* The symmetry-reduced residual (PYMES_SYM_LADDER | PYMES_SYM_RINGS) in its shardable form, one process per
 * GPU.  pymes_residual_slab computes what rank `rank` of `world` owns: the rows [c0,c1) of ETd and ETx (both
 * [o*v][o*v] on the device; ET[(b,j),(a,i)] = Ex[(a,i),(b,j)], rows cut into `world` chunks of ceil(ov/world))
 * and, if L_dev is not NULL, its chunk of rows of the pair-packed ladders L (pymes_ladder_sym with the hole ladder included).  No
 * communication is needed to produce a slab.  After the slabs have been exchanged (one all-gather per buffer)
 * pymes_residual_finish adds the replicated terms and assembles R.  world = 1 reproduces
 * pymes_doubles_residual.  pymes_ccsd_dress_abcd_rows dresses only rows a in [a_begin,a_end) of V_abcd
 * (ccsd.py:414-419) — the rows a rank's ladder chunk reads; with lower_only != 0 only the entries b <= a
 * (all the pair-packed ladder touches) are defined afterwards.
 *
 * t1_dev / QK_dev (both or neither; CCSD/DCSD with PYMES_USE_DRESSED): the T1 dressing of V_abcd (ccsd.py:414-419)
 * is applied on the amplitude side instead — V~_abcd T = sum_pq X_a^p X_b^q V_pqcd T_cdij is evaluated from the
 * undressed, once-packed V_abcd / V_kbcd / V_klcd with tau = T + t1 t1.  V_abcd is then never dressed (no
 * pymes_ccsd_dress_abcd_rows, no second copy of V_abcd) and neither is V_abij: pymes_residual_finish reads it
 * undressed and adds its T1 dressing through Ex + Ex^T as V_abcj t_ci - t_ak (V_kbij + V_kbcj t_ci + V_kbid t_dj + Q_kbij)
 * (the (k,l)-bra part rides in the hole ladder taken with tau).  Only V~_klij, V~_iajb, V~_iabj have to be dressed.
 * QK is a fourth exchange buffer, [o*v][o*o] on the device cut into the same row chunks
 * as ETd: QK[(k,b)][i][j] = sum_cd V_kbcd tau_cdij + V_kbij + V_kbcj t_ci + V_kbid t_dj — the whole bracket above, formed
 * only for the rows (k,b) of the rank. */
int pymes_residual_slab(pymes_ctx* ctx, const double* f_dev, const double* t2_dev, double* ETd_dev, double* ETx_dev,
                        double* L_dev, int rank, int world, uint32_t flags, const double* t1_dev, double* QK_dev,
                        const double* P_dev);
/* P_dev (optional, amplitude-side mode only): the slab's small replicated intermediates — w Tt_cdil V_lkdc (the V.T part
 * of X_ki, ccd.py:215-220) and the pair-packed 2 V_klcd T_cdij of the hole ladder (:180) — as produced by
 * pymes_slab_prepare (every rank sums over its chunk of c / of the pairs (c,d)) and all-reduced by the caller;
 * pymes_slab_prepare_ws doubles.  NULL: the slab forms them itself.
 * One rank with all columns and P_dev == NULL: the rows of ETd / ETx also carry X_ac T_cbij - X_ki T_abkj (ccd.py:231-232),
 * added through the operands of the ring products; the context remembers (t2_dev, ETd_dev) until its next
 * pymes_residual_slab call that does not skip the rings, and pymes_residual_finish[_pairs] ON THE SAME CONTEXT with that
 * t2_dev and that ETd_dev does not add X_ac T again.  Such rows must be finished by the context that made them
 * (PYMES_RING_FOLD=0: the separate products, rows as before). */
int pymes_slab_prepare_ws(pymes_ctx* ctx, int64_t* n_doubles);
int pymes_slab_prepare(pymes_ctx* ctx, const double* t2_dev, double* P_dev, int rank, int world, uint32_t flags);
int pymes_residual_finish(pymes_ctx* ctx, const double* f_dev, const double* t2_dev, const double* ETd_dev,
                          const double* ETx_dev, const double* L_dev, double* r2_dev, uint32_t flags,
                          const double* t1_dev, const double* QK_dev);
int pymes_ccsd_dress_abcd_rows(pymes_ctx* ctx, const double* t1_dev, int a_begin, int a_end, int lower_only);
/* Pair-sharded tail of the iteration (world > 1).  Rank r owns the virtual pairs P(a,b) = a(a+1)/2+b, a >= b, of chunk
 * r of v(v+1)/2 (ceil(npp/world) pairs per chunk, the rows of L it produced in pymes_residual_slab) and keeps every
 * amplitude-sized quantity only for them, in the compact layout Xc[P - r0][2][o*o]: tile 0 = X[a,b,:,:], tile 1 =
 * X[b,a,:,:] (zeros for a == b, so that dots over Xc summed over the ranks equal dots over the full array).
 *   pymes_residual_finish_pairs: pymes_residual_finish restricted to the rank's pairs -> Rc (L is read locally and is
 *                                NOT exchanged; ETd, ETx (and QK) must have been all-gathered); t1/QK NULL for CCD/DCD
 *   pymes_cc_update_pairs:       ccsd.py:176-179 on compact tiles (dt = r/(D+shift), t += delta dt)
 *   pymes_pairs_pack:            compact tiles of this rank from a full [v,v,o,o] array
 *   pymes_pairs_unpack:          full [v,v,o,o] array from the all-gathered compact buffer [world * chunk][2][o*o] */
int pymes_residual_finish_pairs(pymes_ctx* ctx, const double* f_dev, const double* t2_dev, const double* ETd_dev,
                                const double* ETx_dev, const double* L_dev, double* Rc_dev, uint32_t flags,
                                const double* t1_dev, const double* QK_dev, int rank, int world, const double* Xvv_dev);
/* Small replicated intermediates as K-sharded partial sums (world > 1): every rank sums over its chunk of one occupied
 * index and the v x v / o x v results are all-reduced by the caller.
 *   pymes_xvv_partial:              X_ac = f_ac - w Tt_adkl V_lkdc (ccd.py:206-221), k in the rank's chunk, f on rank 0;
 *                                   the all-reduced matrix is handed to pymes_residual_finish_pairs (Xvv_dev, else NULL)
 *   pymes_ccsd_dress_fock_partial:  the six T1.V intermediates of ccsd.py:226-288 (j in the rank's chunk) into W_dev
 *                                   (pymes_ccsd_dress_fock_ws doubles); pymes_ccsd_dress_fock_finish completes f~ from the
 *                                   all-reduced W.  pymes_ccsd_dress_fock = partial(0, 1) + finish. */
int pymes_xvv_partial(pymes_ctx* ctx, const double* f_dev, const double* t2_dev, double* Xvv_dev, int rank, int world,
                      uint32_t flags);
int pymes_ccsd_dress_fock_ws(pymes_ctx* ctx, int64_t* n_doubles);
int pymes_ccsd_dress_fock_partial(pymes_ctx* ctx, const double* t1_dev, double* W_dev, int rank, int world);
int pymes_ccsd_dress_fock_finish(pymes_ctx* ctx, const double* f_dev, const double* t1_dev, const double* W_dev,
                                 double* fd_dev);
int pymes_cc_update_pairs(pymes_ctx* ctx, double* tc_dev, double* dtc_dev, const double* rc_dev, double level_shift,
                          double delta, int rank, int world);
int pymes_pairs_supported(pymes_ctx* ctx, int* yes);   /* the o x o tile of the fused pair kernels fits the LDS */
int pymes_pairs_pack(pymes_ctx* ctx, const double* full_dev, double* xc_dev, int rank, int world);
int pymes_pairs_unpack(pymes_ctx* ctx, const double* xc_all_dev, double* full_dev, int world);
/* ccsd.py:176-179 / ccd.py:123-124: dt = r/(D+shift) (as r * (1/(D+shift))), t += delta*dt; rank 2 or 4 */
int pymes_cc_update(pymes_ctx* ctx, double* t_dev, double* dt_dev, const double* r_dev, double level_shift,
                    double delta, int rank);
/* out-of-place form of the same update: dt = r/(D+shift), t_out = t_in + delta*dt (t_out may alias t_in).  Lets the
 * residuals read T from a fixed buffer (launch graphs) while the DIIS history keeps the updated copy. */
int pymes_cc_update_to(pymes_ctx* ctx, double* t_out_dev, double* dt_dev, const double* t_in_dev, const double* r_dev,
                       double level_shift, double delta, int rank);
/* ccsd.py:458-466 (ccd.py:256-262 when f_dev and t1_dev are NULL) and the norms of ccsd.py:196-197 in ONE pass over
 * T2: out[6] = {one-body, direct, exchange, |t2|^2, |dt2|^2, |t1|^2} (dt2_dev may be NULL); one host synchronisation.
 * |t1|^2 == 0 exactly (the MP2 start; every iteration of a momentum-conserving system such as the UEG) lets the caller take
 * the T1-free form of the residual: exp(-T1) H exp(T1) = H then, no dressing at all (pymes_amd/solver/ccsd.py). */
int pymes_energy_norms(pymes_ctx* ctx, const double* f_dev, const double* t1_dev, const double* t2_dev,
                       const double* dt2_dev, double* out_host);
/* pymes_energy_norms in two halves.  The reference reads the energy back every iteration (ccsd.py:189-197) and its next
 * residual build waits for that; here _start enqueues the reduction and a copy into a pinned slot (`*slot`), the caller may
 * enqueue more work — the residual kernels of the NEXT iteration, which need the new amplitudes but not the energy — and
 * _wait blocks until that one copy has landed (an event, not the stream).  pymes_readback_start / _wait: the same for any
 * n <= 128 doubles of device memory (the DIIS coefficients for the log lines of pymes/mixer/diis.py:104-111); 16 slots per
 * device, reused in turn. */
int pymes_energy_norms_start(pymes_ctx* ctx, const double* f_dev, const double* t1_dev, const double* t2_dev,
                             const double* dt2_dev, int* slot);
int pymes_energy_norms_wait(pymes_ctx* ctx, int slot, double* out_host);
int pymes_readback_start(pymes_ctx* ctx, const double* dev_ptr, int n, int* slot);
int pymes_readback_wait(pymes_ctx* ctx, int slot, double* out_host, int n);
/* The same six sums over the virtual pairs of rank `rank` of `world` only, from the compact tiles [pairs][2][o*o] of the
 * pair-sharded tail (tc_dev, dtc_dev: pymes_pairs_pack layout): partial sums that the caller all-reduces — the energy of
 * ccsd.py:458-466 / ccd.py:256-262 then needs no replicated T2, so the all-gather of the new amplitudes can fly while the
 * next iteration's T1-only work runs.  The T1 sums out[0], out[5] are non-zero on rank 0 only. */
int pymes_energy_norms_pairs(pymes_ctx* ctx, const double* f_dev, const double* t1_dev, const double* tc_dev,
                             const double* dtc_dev, int rank, int world, double* out_host);

/* ---- one process per GPU as WHOLE STEPS, with the collectives of the host program -----------------------------------------
 * The call sequence above (slab, exchange, finish) leaves the collectives to the caller; here the caller hands the library a
 * table of them once and the loop body of ccsd.py:159-197 for one rank becomes three calls — the N > 1 form is expressible
 * from any host language, no Python and no torch involved (the Python host of this repository fills the table with
 * torch.distributed calls, pymes_amd/dist.py:Collectives; an RCCL host with ncclAllReduce / ncclAllGather on a communicator
 * and a stream of its own).
 *
 * Contract of the table.  All buffers are DEVICE memory; `stream` is the stream the library runs on (hipStream_t).
 *   allreduce_start(user, buf, n, stream, &ticket)      in-place sum over the ranks of n doubles at buf
 *   allgather_start(user, buf, chunk, stream, &ticket)  buf = world consecutive chunks of `chunk` doubles, chunk `rank` is
 *                                                       filled in: on completion every rank holds every chunk
 *   wait(user, ticket, stream)                          orders `stream` behind the completion of that collective
 * Each *_start orders its collective behind the work ALREADY enqueued on `stream` and returns without waiting (the usual
 * RCCL pattern: record an event on `stream`, make the communication stream wait for it, enqueue the collective there, record
 * its completion event; wait = hipStreamWaitEvent(stream, that event)).  Tickets are the host program's.  A blocking
 * implementation (synchronise, exchange through host memory, return) is equally valid — the test rigs do that over gloo.
 * Collectives are issued in the same order on every rank.  Return 0 for success; anything else fails the library call.
 *   mark(user, phase)   optional (may be NULL): called at the phase boundaries of a step, for profiling. */
typedef struct pymes_collectives {
    void* user;
    int rank, world;
    int (*allreduce_start)(void* user, double* buf_dev, int64_t n, void* stream, int64_t* ticket);
    int (*allgather_start)(void* user, double* buf_dev, int64_t chunk, void* stream, int64_t* ticket);
    int (*wait)(void* user, int64_t ticket, void* stream);
    void (*mark)(void* user, const char* phase);
} pymes_collectives;
/* the table is copied; NULL removes it.  One table per context (= per GPU = per process). */
int pymes_set_collectives(pymes_ctx* ctx, const pymes_collectives* table);
/* Buffers that take part in a collective belong to the caller (a host that registers memory with its communicator does so
 * once).  With chunk(n) = ceil(n / world), doubles each (pymes_shard_buffer_sizes fills sizes[10] in this order):
 *   ETd, ETx  world chunk(o v) x o v      rows of the ring products (pymes_residual_slab), all-gathered
 *   L         world chunk(v(v+1)/2) x o^2 pair-packed ladder rows (stay on the rank)
 *   QK        world chunk(o v) x o^2      Q_kb rows, all-gathered
 *   Tall      world chunk(v(v+1)/2) x 2 o^2   compact tiles of the new T2, all-gathered
 *   W         pymes_ccsd_dress_fock_ws,  Xvv  v^2,  P  pymes_slab_prepare_ws,  R1  v o   partial sums, all-reduced
 *   S         8                           the six energy / norm sums, all-reduced */
typedef struct pymes_shard_buffers {
    double *ETd, *ETx, *L, *QK, *Tall, *W, *Xvv, *P, *R1, *S;
} pymes_shard_buffers;
int pymes_shard_buffer_sizes(pymes_ctx* ctx, int world, int64_t* sizes_out);
/* ccsd.py:161-171 for this rank (symmetry-reduced form: V_pqrs = V_qpsr, T_abij = T_baji; pymes_pairs_supported): dressed
 * Fock matrix into fd_dev [n,n] + the dressed blocks of the rank's slab, ring products (their rows exchanged while the ladders
 * run), ladders, Q_kb, X_ac, the singles residual (all-reduced: complete in buffers->R1 [v,o] on every rank) and the doubles
 * residual of the rank's virtual pairs as compact tiles rc_dev [max(pairs,1)][2][o*o] (pymes_pairs_pack layout; zero on a rank
 * without pairs).  t2_dev [v,v,o,o] is the replicated array: an exchange left in flight by pymes_ccsd_sharded_finish is
 * completed into it before it is read.  Writes nothing but fd_dev, rc_dev and the buffers, and reads nothing from the host:
 * the caller may enqueue it BEFORE it reads the previous pass's energy (pymes_ccsd_sharded_energy).  The update follows with
 * pymes_cc_update (t1, R1) and pymes_cc_update_pairs (tc, rc), a mixer with pymes_dots / pymes_diis_solve / pymes_lincomb over
 * the compact tiles (overlaps summed over the ranks by the caller), as in the single-rank sequence.  flags: PYMES_DCD. */
int pymes_ccsd_sharded_residuals(pymes_ctx* ctx, const double* f_dev, double* fd_dev, const double* t1_dev, double* t2_dev,
                                 const pymes_shard_buffers* buffers, uint32_t flags, double* rc_dev);
/* ccsd.py:189-197 and the hand-over of the new amplitudes (after the caller's mixer, if any, has replaced t1 / tc): the six
 * sums of pymes_energy_norms_pairs all-reduced ON THE DEVICE and copied to the host on the side (`*slot`, read with
 * pymes_ccsd_sharded_energy — after the caller has enqueued the next pymes_ccsd_sharded_residuals if it wishes: nothing on the
 * stream waits for the host), tc into the exchange buffer, the all-gather of the new T2 started.  It is completed by the next
 * pymes_ccsd_sharded_residuals, or by pymes_ccsd_sharded_await (end of the solve: t2_dev then holds the amplitudes). */
int pymes_ccsd_sharded_finish(pymes_ctx* ctx, const double* f_dev, const double* t1_dev, const double* tc_dev,
                              const double* dtc_dev, const pymes_shard_buffers* buffers, int* slot);
int pymes_ccsd_sharded_energy(pymes_ctx* ctx, int slot, double* out_host /* [6], as pymes_energy_norms */);
int pymes_ccsd_sharded_await(pymes_ctx* ctx, double* t2_dev, const pymes_shard_buffers* buffers);
/* CCD / DCD (pymes/solver/ccd.py:93-150; the reference's UEG drivers, BASELINE config 4) as the same whole steps: the loop body
 * of ccd.py:100-121 for this rank — ring products (their rows exchanged while the ladders run), ladders, the doubles residual
 * of the rank's virtual pairs as compact tiles rc_dev.  There is no T1: nothing is dressed, no singles residual; of `buffers`
 * only ETd, ETx, L, Tall and S are used (the others may be NULL).  The pass is completed by pymes_cc_update_pairs, the mixer
 * and pymes_ccsd_sharded_finish / _energy / _await with f_dev = t1_dev = NULL.  flags: PYMES_DCD, PYMES_OWNER_TILES. */
int pymes_ccd_sharded_residuals(pymes_ctx* ctx, const double* f_dev, double* t2_dev, const pymes_shard_buffers* buffers,
                                uint32_t flags, double* rc_dev);
/* OWNER TILES (flag PYMES_OWNER_TILES of pymes_ccsd_sharded_residuals / pymes_ccd_sharded_residuals).  In the pair-sharded
 * tail rank q assembles R only for its virtual pairs P(a,b), a in [a0,a1), and reads of ETd / ETx just the tiles [(a,.),(b,.)]
 * and [(b,.),(a,.)]: rows [0, a1 o) x columns [a0 o, a1 o) and rows [a0 o, a1 o) x columns [0, a0 o).  ONE all-to-all of those
 * rectangles ((50,200) on 8 ranks: 1.06 GB per iteration on the wire instead of 2.33) replaces the two all-gathers.  The host
 * program adds an all-to-all to its table —
 *   alltoallv_start(user, send_dev, send_counts[world], recv_dev, recv_counts[world], stream, &ticket)
 * counts in doubles, the pieces for / from rank 0, 1, ... contiguous in that order in send_dev / recv_dev (ncclSend / ncclRecv
 * in a group, or MPI_Alltoallv with running offsets); ordering and tickets as for the other collectives — and hands over two
 * staging buffers of pymes_owner_tile_sizes doubles.  The library packs and unpacks the rectangles itself. */
#define PYMES_OWNER_TILES (1u << 21)
typedef int (*pymes_alltoallv_fn)(void* user, const double* send_dev, const int64_t* send_counts, double* recv_dev,
                                  const int64_t* recv_counts, void* stream, int64_t* ticket);
int pymes_set_alltoallv(pymes_ctx* ctx, pymes_alltoallv_fn fn /* NULL removes it */);
int pymes_owner_tile_sizes(pymes_ctx* ctx, int rank, int world, int64_t* send_doubles, int64_t* recv_doubles);
int pymes_set_owner_tile_buffers(pymes_ctx* ctx, double* send_dev, double* recv_dev);
/* CCSD.get_energy, ccsd.py:458-466: e_out = {one-body, direct, exchange}; f is the UNDRESSED Fock */
int pymes_ccsd_energy(pymes_ctx* ctx, const double* f_dev, const double* t1_dev, const double* t2_dev,
                      double* e_out_host);
/* CCD.get_energy, ccd.py:256-262: e_out = {direct, exchange} */
int pymes_ccd_energy(pymes_ctx* ctx, const double* t2_dev, double* e_out_host);

/* ---- uniform electron gas integrals: UEG.eval_2b_integrals, pymes/model/ueg.py:265-516 ---------------- */
/* V_dev[n_p^4] = <pq|rs> of the plane-wave basis k_int_host[n_p][3] (sorted by kinetic energy, as
 * UEG.init_single_basis builds it) with lookup table index_map_host[(2 imax + 1)^3] (basis_indices_map).
 * mode 0: Coulomb (correlator None); 1: transcorrelated is_only_2b; 2: is_effect_2b BEFORE its
 * electron-exchange symmetrisation (ueg.py:509-513: use pymes_permute); 3: is_rpa_approx.  The correlator is
 * UEG.trunc (ueg.py:772-800) with parameters k_cutoff, gamma; lattice_cutoff is sumNablaUSquare's (30). */
int pymes_ueg_eval_2b(pymes_ctx* ctx, int n_p, int n_ele, int imax, int mode, double L, double k_cutoff, double gamma,
                      int lattice_cutoff, const int32_t* k_int_host, const int32_t* index_map_host, double* V_dev);

/* The same with the reference's other correlators, evaluated inside the kernels from the same float k^2 the reference forms
 * (so that a cut-off lying exactly on a lattice shell is resolved the way the reference's roundings resolve it):
 * correlator 1 UEG.gaskell (ueg.py:836-883) params {mu, cut}, 2 gaskell_modified (:802-834) {cut}, 3 coulomb (:905-915)
 * {-4 pi gamma}, 4 yukawa (:740-770) {gamma, floor}, 5 stg (:917-935) {gamma^2, floor, -4 pi / gamma}, 6 smooth (:885-903)
 * {kc, kc gamma, (kc gamma)^2}; params[4], derived from the model by pymes_amd/model/ueg.py with the reference's expressions. */
int pymes_ueg_eval_2b_corr(pymes_ctx* ctx, int n_p, int n_ele, int imax, int mode, double L, int lattice_cutoff,
                           int correlator, const double* params_host, const int32_t* k_int_host,
                           const int32_t* index_map_host, double* V_dev);
/* The same for a correlator u(k^2) of the caller's own (any Python callable): every argument of u is |2 pi n / L|^2 for an integer vector n, so u is handed over as
 * two host tables over m = |n|^2 (tab_len >= 3 (lattice_cutoff + 2 imax)^2 + 1): tab_scalar[m] is what the reference's
 * correlator returns when called with a float (the main loop's `d_k_vec.dot(d_k_vec)`, ueg.py:409), tab_array[m] what it
 * returns when called with an ndarray (everything else: sumNablaUSquare, the 3-body contractions) — the two forms of
 * `gaskell` differ at its cut-off.  modes 1-3 as above. */
int pymes_ueg_eval_2b_tab(pymes_ctx* ctx, int n_p, int n_ele, int imax, int mode, double L, int lattice_cutoff,
                          const int32_t* k_int_host, const int32_t* index_map_host, const double* tab_scalar_host,
                          const double* tab_array_host, int64_t tab_len, double* V_dev);
/* The same elements for a list: out_dev[t] = <pq|rs> of pqrs_dev[t][4] (int32, device), t < count -- the integral sectors of
 * the momentum-sector solver (below), never a dense array.  One entry for all correlators: tab_array_host non-NULL selects the
 * tables (with tab_scalar_host, tab_len as above), else correlator 0 is UEG.trunc with (k_cutoff, gamma) and 1..6 the named
 * ones with params_host[4].  Momentum conservation is decided in exact integer arithmetic: an entry that does not conserve
 * the vector is 0 (the dense builder range-checks only the flattened lookup index, like the reference, and sets a few such
 * elements at some bases); an entry that names no orbital is NaN.  mode 2 is written already symmetrised,
 * (E[p,r] + E[q,s]) / 2.  Synchronises; refused while a launch graph is being recorded. */
int pymes_ueg_eval_2b_list(pymes_ctx* ctx, int n_p, int n_ele, int imax, int mode, double L, double k_cutoff, double gamma,
                           int lattice_cutoff, int correlator, const double* params_host, const int32_t* k_int_host,
                           const double* tab_scalar_host, const double* tab_array_host, int64_t tab_len,
                           const int32_t* pqrs_dev, int64_t count, double* out_dev);
/* The state that list form prepares (the kernel parameters, the correlator tables, for mode 1 the u_mat table with its index, for
 * mode 2 E[p,r]), kept on the device as a ladder term: the element a term defines for (p,q,r,s) is exactly what
 * pymes_ueg_eval_2b_list with the same arguments writes for that entry, bit for bit -- both run one device function.  The
 * arguments are those of the list form up to tab_len.  *term is an opaque handle of this context: pymes_ueg_ladder_term_free
 * releases it, and so does pymes_ctx_destroy for every term still alive.  pymes_ueg_ladder_term_bytes: the device bytes a term
 * holds (nothing for modes 0 and 3 without tables, ~ 8 n_p^2 for mode 2).  create synchronises and is refused while a launch
 * graph is being recorded. */
int pymes_ueg_ladder_term_create(pymes_ctx* ctx, int n_p, int n_ele, int imax, int mode, double L, double k_cutoff, double gamma,
                                 int lattice_cutoff, int correlator, const double* params_host, const int32_t* k_int_host,
                                 const double* tab_scalar_host, const double* tab_array_host, int64_t tab_len, void** term);
int pymes_ueg_ladder_term_free(pymes_ctx* ctx, void* term);
int pymes_ueg_ladder_term_bytes(pymes_ctx* ctx, const void* term, int64_t* bytes);

/* ---- momentum-sector CCD / DCD (pymes_amd/solver/ueg_cc.py, sectors.py; DESIGN "Momentum sectors") -------------
 * A Hamiltonian whose orbitals carry a conserved integer vector keeps ~ o^2 v amplitudes, held block by block (one block
 * per pair momentum, or per momentum transfer); every contraction of ccd.py:164-254 is one ragged batch of small products.
 *
 * pymes_sector_gemm: C[c..] = alpha op(A[a..]) op(B[b..]) + beta C[c..] for every record of a DEVICE-RESIDENT task table:
 * row-major operands at element offsets a, b, c of the three arenas, leading dimensions lda, ldb, ldc, op = transpose when
 * the flag is set (A is then stored k x m, B n x k).  m, n, k >= 0 (an empty block is legal; k = 0 scales C by beta).  One
 * workgroup takes one PYMES_SECTOR_TILE_M x PYMES_SECTOR_TILE_N tile of one output block; tile0 is the number of tiles of
 * all earlier records and ntiles their total.  No atomics, k summed in ascending order: identical calls give identical
 * bits.  The kernel trusts the table (pymes_amd/solver/sectors.py checks it against the arena lengths before the upload);
 * nothing outside the blocks is read or written, with beta = 0 the output block is not read, and C must not overlap A or B. */
#define PYMES_SECTOR_TILE_M 32
#define PYMES_SECTOR_TILE_N 16
#define PYMES_SECTOR_TRANS_A 1
#define PYMES_SECTOR_TRANS_B 2
typedef struct pymes_sector_task {
    int64_t m, n, k;
    int64_t a, b, c;
    int64_t lda, ldb, ldc;
    int64_t flags;
    int64_t tile0;
    double alpha, beta;
    int64_t reserved;
} pymes_sector_task;
int pymes_sector_gemm(pymes_ctx* ctx, const pymes_sector_task* tasks_dev, int ntask, int64_t ntiles, const double* A_dev,
                      const double* B_dev, double* C_dev);
/* The direct particle ladder: C^t = alpha op(A^t) B^t + beta C^t for every record of a device-resident task table, with
 *   A^t[(a,b),(c,d)] = sum_{q < nterms} coef_host[q] w_q(a,b,c,d)
 * never read from memory: w_q is the element of ladder term q (above) and (a,b), (c,d) are the entries first_dev[t] + row and
 * first_dev[t] + column of vv_rows_dev, the vv pair list as absolute orbital indices (int32 [rows, 2], the order of
 * SectorTables.vv_pairs); first_dev: int64, one per task; k_int_dev: int32 [n_p, 3].  Of a record m, n, k, b, c, ldb, ldc,
 * alpha, beta, tile0 and PYMES_SECTOR_TRANS_A are used (tile0 and ntiles as pymes_sector_gemm counts them, whatever tile the
 * kernel takes); a and lda are ignored.  With TRANS_A the element at output row (a,b) and summation index (c,d) is w(c,d,a,b).
 * Contract: every output element adds its k products in ascending order with fma from +0.0 and ends with the rounded
 * alpha acc (+ rounded beta C) of pymes_sector_gemm -- for one term with coefficient 1 the result has the bits of
 * pymes_sector_gemm on the stored block.  Several terms are combined as pymes_lincomb combines stored arenas, s = 0 then
 * s = s + w_q coef_q in ascending q with product and sum rounded separately: the bits of the stored sum for sums of terms that
 * were each scaled at most once (coefficients that are powers of two: any order of scaling and adding).  No atomics; identical
 * calls give identical bits; nothing outside m, n, k is read or written; with beta = 0 the output is not read.  The kernel
 * trusts the task table, first_dev and vv_rows_dev (pymes_amd/solver/ueg_cc.py checks them before the upload).  Refused: more
 * than PYMES_SECTOR_LADDER_MAX_TERMS terms, a term of another context or of another n_p, terms of different L. */
#define PYMES_SECTOR_LADDER_MAX_TERMS 4
int pymes_sector_ladder_direct(pymes_ctx* ctx, const pymes_sector_task* tasks_dev, int ntask, int64_t ntiles,
                               const int64_t* first_dev, const int32_t* vv_rows_dev, const int32_t* k_int_dev, int n_p, int nterms,
                               void* const* terms, const double* coef_host, const double* B_dev, double* C_dev);
/* dst[i] = beta dst[i] + a1 s1[m1[i]] + a2 s2[m2[i]], i < n (int64 maps on the device; s2_dev NULL: one source; beta = 0: dst
 * is not read).  The moves between the three sector layouts, 2 D - C among them. */
int pymes_sector_gather(pymes_ctx* ctx, double* dst_dev, int64_t n, double beta, double a1, const double* s1_dev,
                        const int64_t* m1_dev, double a2, const double* s2_dev, const int64_t* m2_dev);
/* The diagonal X_ac / X_ki terms (ccd.py:213-235) in the direct layout, rows g = (a,i) of row_len[g] elements from
 * row_start[g] on: s[g] = sum_c Tt[g,c] W1[g,c] in ascending c, x_oo[i] = eps[i] + w sum_a s, x_vv[a] = eps[no + a] - w sum_i s,
 * Ex[g,:] += (x_vv[a] - x_oo[i]) D[g,:].  row_of[a no + i] = g and ai_of[g] = a no + i; ws_dev: no nv + no + nv doubles. */
int pymes_sector_xdiag(pymes_ctx* ctx, const double* Tt_dev, const double* W1_dev, const double* D_dev, double* Ex_dev,
                       const double* eps_dev, double w, int no, int nv, const int64_t* row_start_dev, const int64_t* row_len_dev,
                       const int64_t* row_of_dev, const int64_t* ai_of_dev, double* ws_dev);
/* dt = r / (den + shift), t_out = t_in + dt over n elements (t_in_dev NULL: t_out = dt, the MP2 start; dt_dev NULL: not kept) */
int pymes_sector_update(pymes_ctx* ctx, double* t_out_dev, double* dt_dev, const double* t_in_dev, const double* r_dev,
                        const double* den_dev, double shift, int64_t n);
/* Momentum-blocked (T) (pymes_amd/solver/ueg_cc.py, sector_triples_energy): *e_out_host = sum of m_ijk S_ijk over
 * the unique occupied triples [t_begin, t_end) in the order of pymes_ccsd_t (i ascending, j <= i, k <= j,
 * t = i(i+1)(i+2)/6 + j(j+1)/2 + k), for amplitudes without singles.  Momentum conservation leaves one term in each sum of
 * w_ijk, so the operands come with their implied index left out (sectors.TriplesTables), virtuals counted from no:
 *   Vv[i,a,b] = V[i,f*,a,b] [o,v,v]   Vo[i,j,a] = V[i,j,a,m*] [o,o,v]   Tc[i,j,a] = T[a,b*,i,j] [o,o,v]   m_of[i,j,a] = m* or -1
 * with an exact 0 wherever the implied orbital does not exist (the kernel relies on it).  k_int_dev: int32 [no + nv, 3];
 * orb_of_dev: the int32 lookup grid vector -> orbital (-1: none) over the box box_host = {lo[3], dims[3]}, row-major; a
 * vector outside the box names no orbital.  With c the virtual of k_i + k_j + k_k - k_a - k_b (if any),
 *   Wt[a,b] = w(ijk;abc) + w(ikj;acb) + w(jik;bac) + w(jki;bca) + w(kij;cab) + w(kji;cba),
 *   w(xyz;pqr) = Vv[x,p,q] Tc[z,y,r] - (m = m_of[x,y,p]) >= 0 ? Vo[x,y,p] Tc[m,z,q] : 0,
 *   S = 1/3 sum_{a,b: c} Wt[a,b] (4 Wt[a,b] + Wt[b,c] + Wt[c,a] - 2 Wt[c,b] - 2 Wt[a,c] - 2 Wt[b,a]) / (e_i + e_j + e_k - e_a - e_b - e_c).
 * The range is worked off in batches of as many triples as ws_bytes hold, nv^2 + ceil(nv / 32)^2 + 1 doubles each (a workspace
 * below one triple is refused); every slab element that is read is written in the same call.  No atomics: one partial per
 * workgroup, added in index order; the value of a triple has the same bits for every batch size, range and repetition, and
 * the sum adds the values in triple order, carrying the rounding error of every add along
 * (Neumaier), so it is the exactly rounded sum of the values but for the last unit.  per_triple_dev (t_end - t_begin doubles) may be NULL.  The kernels trust m_of < no
 * and orb_of < no + nv.  Synchronises; refused while a launch graph is being recorded. */
int pymes_sector_triples(pymes_ctx* ctx, int no, int nv, const double* eps_dev, const int32_t* k_int_dev, const int32_t* orb_of_dev,
                         const int32_t* box_host, const int32_t* m_of_dev, const double* Tc_dev, const double* Vv_dev,
                         const double* Vo_dev, int64_t t_begin, int64_t t_end, double* ws_dev, int64_t ws_bytes,
                         double* per_triple_dev, double* e_out_host);
/* Momentum-blocked Lambda-(T) (pymes_amd/solver/ueg_cc.py, sector_lambda_triples_energy): the triples correction for
 * integrals without V_pqrs = V_rspq, lam1 = 0 (singles vanish on the sectors).  Arguments, triple order, tables, lookup box and
 * the exact-zero contract as pymes_sector_triples, with two slabs per triple:
 *   WR[a,b] = the Wt of pymes_sector_triples from VvR[i,a,b] = V[a,b,i,f*], VoR[i,j,a] = V[a,m*,i,j] and Tc
 *   WL[a,b] = the same from VvL[i,a,b] = V[i,f*,a,b], VoL[i,j,a] = V[i,j,a,m*] and Lc[i,j,a] = L[a,b*,i,j],
 *             L = (2 lambda2 + lambda2^x) / 3, lambda2^x[a,b,i,j] = lambda2[b,a,i,j]
 *   S = 1/3 sum_{a,b: c} WR[a,b] (4 WL[a,b] + WL[b,c] + WL[c,a] - 2 WL[c,b] - 2 WL[a,c] - 2 WL[b,a]) / (e_i + e_j + e_k - e_a - e_b - e_c).
 * ws_bytes hold 2 nv^2 + ceil(nv / 32)^2 + 1 doubles per triple of a batch (below one triple: refused).  No atomics; the
 * value of a triple has the same bits for every batch size, range and repetition; the sum is the Neumaier sum in triple
 * order.  Synchronises; refused while a launch graph is being recorded. */
int pymes_sector_triples_lambda(pymes_ctx* ctx, int no, int nv, const double* eps_dev, const int32_t* k_int_dev,
                                const int32_t* orb_of_dev, const int32_t* box_host, const int32_t* m_of_dev, const double* Tc_dev,
                                const double* Lc_dev, const double* VvR_dev, const double* VoR_dev, const double* VvL_dev,
                                const double* VoL_dev, int64_t t_begin, int64_t t_end, double* ws_dev, int64_t ws_bytes,
                                double* per_triple_dev, double* e_out_host);
/* Sector densities (pymes_amd/solver/ueg_cc.py, SectorDensity).
 * pymes_sector_bin_sums: out[b] = beta out[b] + alpha sum_j src[list[j]], off[b] <= j < off[b + 1], b < nbins (int64 CSR on the
 * device: nbins + 1 offsets; the sums of a density arena over the bins of the momentum transfer).  A workgroup owns four
 * consecutive bins; a bin of at most 256 elements is summed by one wavefront, a longer one by the whole workgroup; each
 * thread adds in ascending list order, then a fixed tree.  No atomics: identical calls give identical bits.  An empty bin
 * gives alpha 0 (+ beta out[b]); with beta = 0 out is not read.  The kernel trusts the lists (the host checks them). */
int pymes_sector_bin_sums(pymes_ctx* ctx, double* out_dev, int64_t nbins, const int64_t* off_dev, const int64_t* list_dev,
                          const double* src_dev, double alpha, double beta);
/* The V_abcd part of the transfer sums, never an array over the v^4 sectors: for every bin vector q = bin_q[b] (int32 [nbins,3])
 *   out[b] = sum over the rows (a,b) of the pp layout with c = orb(k_a + q), d = orb(k_b - q) both virtual of
 *            sum_ij lam[(a,b),ij] T[(c,d),ij].
 * Row r of the pp layout: the virtual pair vv_pairs[r] (int32 [rows,2], counted from the first virtual), row_len[r] contiguous
 * doubles from row_start[r] on in both compact vectors; row_of_pair[c nv + d] is the row of a virtual pair or -1.  k_int_dev,
 * orb_of_dev, box_host: as pymes_sector_triples.  One workgroup owns a bin (at most max_groups workgroups stride over the
 * bins; 0: one per bin); its threads stride over all rows in ascending order, then a fixed tree: no atomics, and the value
 * of a bin has the same bits for every max_groups and every repetition.  A bin no row reaches is an exact +0.0. */
int pymes_sector_pair_transfer(pymes_ctx* ctx, double* out_dev, int64_t nbins, const int32_t* bin_q_dev, const int32_t* k_int_dev,
                               const int32_t* orb_of_dev, const int32_t* box_host, int no, int nv, int64_t rows,
                               const int32_t* vv_pairs_dev, const int64_t* row_start_dev, const int64_t* row_len_dev,
                               const int64_t* row_of_pair_dev, const double* lam_dev, const double* T_dev, int max_groups);
/* gamma of the sector densities from the row sums rho[g] = sum_c x[g,c] y[g,c] of the direct layout (rows as
 * pymes_sector_xdiag): gamma[no + a] = sum_i rho[row(a,i)], gamma[i] = -sum_a rho[row(a,i)], every sum in ascending order.
 * gamma_dev: no + nv doubles; ws_dev: no nv doubles. */
int pymes_sector_gamma(pymes_ctx* ctx, const double* x_dev, const double* y_dev, int no, int nv, const int64_t* row_start_dev,
                       const int64_t* row_len_dev, const int64_t* row_of_dev, double* gamma_dev, double* ws_dev);
/* Sector IP- / EA-EOM-CCD (pymes_amd/solver/ueg_eom.py, SectorIPEASigma): one momentum block of the IP (kind 0) or EA
 * (kind 1) operator of tests/_ipea_reference.py with t1 = 0 and a diagonal Fock matrix, for the target orbital p (an index over
 * all no + nv orbitals: occupied for IP, virtual for EA).  The block is the singles element r1[p] and the doubles with their
 * implied virtual b* left out, at the positions t = x no + y:
 *   IP  R[i,j] = r2[i,j,b*], k_b* = k_i + k_j - k_p, [no,no]        EA  R[a,j] = r2[a,b*,j], k_b* = k_p + k_j - k_a, [nv,no]
 * b_of[t] = b* counted from the first virtual, or -1: such a position is not part of the space.  k_int_dev, orb_of_dev, box_host
 * and the exact-zero contract of Tc, Vv, Vo, VvR, VoR: as pymes_sector_triples / pymes_sector_triples_lambda.  All three are
 * refused while a launch graph is being recorded.
 *
 * pymes_sector_ipea_prepare: what depends on the target alone, every sum in ascending index order.  L_dev: no + nv doubles,
 * L_oo then L_vv (the x of pymes_sector_xdiag with w = 1).  With orbv(q) the virtual that carries q (counted from the first
 * virtual), a term being left out where there is none, and pv = p - no:
 *   IP  d2[t] = L[no + b*] - L[i] - L[j]            W[t] = -2 Vo[j,i,b*] + Vo[i,j,b*]
 *       U[t]  = -VoR[j,i,b*] + sum_k { c = orbv(k_k + k_p - k_i): Vo[k,p,c] (-2 Tc[k,j,c] + Tc[j,k,c]) + Vo[p,k,c] Tc[k,j,c];
 *                                      c = orbv(k_k + k_p - k_j): Vo[p,k,c] Tc[i,k,c] }
 *               - sum_c { orbv(k_i + k_j - k_c) = d: Vv[p,c,d] Tc[i,j,c] }
 *   EA  d2[t] = L[no + a] + L[no + b*] - L[j]       W[t] = 2 Vv[j,b*,a] - Vv[j,a,b*]
 *       U[t]  = VvR[j,b*,a] + sum_k { c = orbv(k_k + k_a - k_p): Vv[k,c,pv] (2 Tc[k,j,c] - Tc[j,k,c]) - Vv[k,pv,c] Tc[k,j,c];
 *                                     c = orbv(k_k + k_b* - k_p): -Vv[k,pv,c] Tc[j,k,c];
 *                                     m the occupied with k_p + k_j - k_k: Vo[k,m,pv] Tc[k,m,a] }
 * and U = W = 0, d2 = outside (finite, non-zero) where b_of[t] < 0.  d2 is the doubles part of the preconditioner's diagonal
 * (d1 = -L[p] / L[p]) and the coefficient of R in s2; U is everything r1 multiplies in s2; s1 = -+ L[p] r1 + sum_t W[t] R[t].
 *
 * pymes_sector_ipea_pack: the k <= 32 vectors r2_dev[z] (npos doubles each) into the operands of the products, the vector index
 * running fastest: XR[ph[t] k + z] = R_z[t], XX[ph[t] k + z] = R_z[partner[t]], XP[pair[t] k + z] = R_z[t] for the positions
 * inside the space.  ph, partner, pair: int64 [npos] on the device, -1 outside the space, bijections of the space onto
 * [0, count) resp. an involution of it (sectors.QuasiparticleTables; the host checks them, the kernels trust them).
 *
 * pymes_sector_ipea_assemble: s2_z[t] = d2[t] R_z[t] + r1_z U[t] + G1[ph[t] k + z] + G2[ph_partner[t] k + z] + H[pair[t] k + z],
 * added in this order, an exact +0.0 outside the space, and s1_z = d1 r1_z + sum_t W[t] R_z[t] (one workgroup per vector:
 * each thread over t = tid, tid + 256, ... ascending, then a fixed tree).  G1 = PA XR + PB XX, G2 = MDU XX (the ring products),
 * H the ladder product of XP, all from pymes_sector_gemm.  r1_dev[z], s1_dev[z] point at one double.  No atomics: identical
 * calls give identical bits, and a vector's sigma does not depend on the others of its call. */
int pymes_sector_ipea_prepare(pymes_ctx* ctx, int kind, int target, int no, int nv, const int32_t* k_int_dev,
                              const int32_t* orb_of_dev, const int32_t* box_host, const int32_t* b_of_dev, const double* L_dev,
                              const double* Tc_dev, const double* Vv_dev, const double* Vo_dev, const double* VvR_dev,
                              const double* VoR_dev, double outside, double* U_dev, double* W_dev, double* d2_dev);
int pymes_sector_ipea_pack(pymes_ctx* ctx, int k, const double* const* r2_dev, int64_t npos, const int64_t* ph_dev,
                           const int64_t* partner_dev, const int64_t* pair_dev, double* XR_dev, double* XX_dev, double* XP_dev);
int pymes_sector_ipea_assemble(pymes_ctx* ctx, int k, const double* const* r1_dev, const double* const* r2_dev,
                               double* const* s1_dev, double* const* s2_dev, int64_t npos, const int64_t* ph_dev,
                               const int64_t* ph_partner_dev, const int64_t* pair_dev, const double* d2_dev, const double* U_dev,
                               const double* W_dev, double d1, const double* G1_dev, const double* G2_dev, const double* H_dev);
/* pymes_eom_correction (below) for flat vectors [x1 (n1) | zero pad | x2] of any lengths, n1 >= 1, off2 >= n1, len > off2: the
 * same kernels.  Refused while a launch graph is being recorded. */
int pymes_sector_ipea_correction(pymes_ctx* ctx, int n, const double* const* s_dev, const double* const* r_dev, const double* w_host,
                                 const double* d_dev, double shift, double* const* q_dev, int64_t n1, int64_t off2, int64_t len,
                                 double* norms_host);

/* One Arnoldi step on a device-resident basis (pymes_amd/solver/ueg_eom.py, SectorSpectralFunction).  The basis is one
 * matrix whose rows lie `pitch` doubles apart (a multiple of 32, at least len) with len valid doubles each; what lies between
 * len and pitch is neither read nor written.  On entry the rows 0..j are orthonormal and row j+1 holds w = H v_j; the call needs
 * j + 2 rows.  hess_dev is row-major with rows ldh doubles apart, ldh >= j + 1, and j + 2 rows are written to.  On exit
 *   hess[i ldh + j] = h_i + h'_i, i <= j, of two rounds of classical Gram-Schmidt (h = V w, w' = w - V^T h, h' = V w',
 *                     w'' = w' - V^T h'),
 *   hess[(j+1) ldh + j] = |w''|  and  row j+1 = w'' / |w''|,
 * or, on breakdown (not |w''| > breakdown |w|), hess[(j+1) ldh + j] = 0.0 exactly, row j+1 = +0.0 everywhere and
 * status_dev[0] = j + 1 if it held 0 (the caller zeroes it before the first step; the first breakdown stays).
 * Nothing is read back and the host does not wait.  No atomics: every dot is a fixed tree whose shape depends on len alone --
 * not on j, pitch, or the rows allocated --, so identical calls give identical bits.  ws_dev: *ws_doubles doubles of scratch;
 * with ws_dev == NULL the call only writes the size that (len, j) need into *ws_doubles (it grows with j) and the other
 * pointers may be NULL.  Refused by name: a null argument, j outside [0, PYMES_SECTOR_ARNOLDI_MAX), len < 1, pitch < len or no
 * multiple of 32, ldh < j + 1, a breakdown threshold that is negative or not finite, a workspace that is too small, and a
 * context that is recording a launch graph. */
#define PYMES_SECTOR_ARNOLDI_MAX 512
int pymes_sector_arnoldi_step(pymes_ctx* ctx, double* basis_dev, int64_t pitch, int64_t len, int j, double* hess_dev, int64_t ldh,
                              double breakdown, double* ws_dev, int64_t* ws_doubles, int64_t* status_dev);

/* ---- vector helpers for DIIS (pymes/mixer/diis.py:65-103) and norms ----------------- */
/* out_host[p] = sum_i x[p][i]*y[p][i], npairs <= 16, deterministic reduction (synchronises) */
int pymes_dots(pymes_ctx* ctx, int npairs, const double* const* x_dev, const double* const* y_dev, int64_t n,
               double* out_host);
/* the same with one length per pair (the DIIS overlaps of T1 and T2 in one launch / one synchronisation) */
int pymes_dots_var(pymes_ctx* ctx, int npairs, const double* const* x_dev, const double* const* y_dev,
                   const int64_t* n, double* out_host);
/* out = sum_k c[k]*x[k], nx <= 8 */
int pymes_lincomb(pymes_ctx* ctx, double* out_dev, int nx, const double* const* x_dev, const double* c_host,
                  int64_t n);
/* Grouped launches of small products.  The reference evaluates its term sequences one einsum after the other
 * (pymes/solver/ccd.py:175-240, eom_ccsd.py:288-383); on the device the small ones are 5-50 us kernels on a quarter-filled
 * chip.  Products (pymes_contract / pymes_dgemm) issued between begin and end are INDEPENDENT by the caller's promise — none
 * reads or accumulates into the output of another — and those that run on 64 x 64 tiles are launched together, up to 16
 * per launch (one launch per dependency level).  Anything else the context enqueues in between launches the queue first.
 * _end reports the grouped launches made and the products they carried (either pointer may be NULL). */
int pymes_gemm_group_begin(pymes_ctx* ctx);
int pymes_gemm_group_end(pymes_ctx* ctx, int64_t* launches, int64_t* products);
/* Tall-skinny subspace algebra of the Davidson driver (pymes/solver/eom_ccsd.py:91 `QR`, :103-109 the subspace matrix
 * B[j,l] = <u_j, w_l>, :122-147 collapse / expansion vectors; reference: numpy on host arrays, vector by vector) and of the
 * FEAST driver (feast_eom_ccsd.py:110-150).  Every vector of a call is read once.
 * pymes_gram: out_host[i*n + j] = <x_i, y_j>, i < m, j < n, vectors of `len` doubles on the device (m, n <= 64);
 * deterministic; synchronises the context's stream.
 * pymes_lincomb_multi: y_j = sum_{i<m} c_host[i*n + j] x_i + beta_host[j] y_j (beta_host NULL = 0; a y_j with beta 0 is
 * never read); an output may be one of the inputs only when m <= 16 and n <= 4. */
int pymes_gram(pymes_ctx* ctx, int m, int n, const double* const* x_dev, const double* const* y_dev, int64_t len,
               double* out_host);
int pymes_lincomb_multi(pymes_ctx* ctx, int m, int n, const double* const* x_dev, const double* c_host,
                        const double* beta_host, double* const* y_dev, int64_t len);
/* One DIIS step (pymes/mixer/diis.py:40-103) with no host round trip.  state_dev: 96 doubles on the device —
 * [0] order of L, [1..81] L (pitch 9), [82..90] coefficients of the last step, [91] 1 if the pseudo-inverse branch
 * (diis.py:85-93) was taken, [92] steps taken; a fresh mixer starts from {1, 0, ...}.  The npairs = ntypes * m overlaps
 * <x_p, y_p> (type-major: p = t * m + i) are reduced on the device, L is shifted / extended (including the reference's
 * full-subspace quirk, diis.py:59-60) and L c = (0,..,0,-1) is solved by one device thread; pymes_lincomb_dev then forms
 * sum_k c[k] x[k] with the coefficients read from state_dev + 82.  Nothing synchronises: the host reads the state
 * (pymes_download) only when it wants to log it. */
/* The same step with the small algebra on the calling host thread: overlaps reduced on the device (one synchronisation),
 * L and the coefficients in state_host (96 doubles, layout as above), the extrapolations out[t] = sum_i c[i] amp_hist[t*m+i]
 * enqueued before the call returns — what the solvers use: the device waits for the host only for the synchronisation itself,
 * not for an interpreter to run numpy.linalg on a 7 x 7 matrix (diis.py:65-103 in one call). */
int pymes_diis_mix(pymes_ctx* ctx, double* state_host, int ntypes, int m, int was_full, const double* const* err_hist_dev,
                   const double* const* err_new_dev, const int64_t* sizes, const double* const* amp_hist_dev,
                   double* const* out_dev);
int pymes_diis_step(pymes_ctx* ctx, double* state_dev, int npairs, const double* const* x_dev, const double* const* y_dev,
                    const int64_t* n, int ntypes, int m, int was_full);
/* Only the small algebra of that step (diis.py:56-103), on the calling host thread and on host arrays: overlaps_host[t * m + i]
 * = <e_i, e_new> of amplitude type t, already complete (one process per GPU: summed over the ranks by the caller).  L and
 * the coefficients in state_host as above; state_host[91] = 2 when L is singular or not finite.  No context, no device. */
int pymes_diis_solve(double* state_host, const double* overlaps_host, int ntypes, int m, int was_full);
int pymes_lincomb_dev(pymes_ctx* ctx, double* out_dev, int nx, const double* const* x_dev, const double* coeff_dev,
                      int64_t n);
/* ---- The amplitude tail of the single-rank loop on EXCHANGE-SYMMETRIC amplitudes.  In that loop every [v,v,o,o] array of
 * the update, the mixer and the energy pass has X_abij == X_baji (T2, dT2, each stored DIIS vector, V_ijab): the calls below
 * are those above with the caller's DECLARATION of that symmetry — never inferred from a shape.  Each pair of tiles (a,b),
 * (b,a) is then read once: the reductions sum the tiles a >= b and count the off-diagonal ones twice; the element-wise
 * steps compute tile (a,b) exactly as the plain call does and store it as (a,b) and, transposed, as (b,a), so their outputs
 * are exchange-symmetric bit for bit (the plain call evaluates tile (b,a) on its own: the two agree to the rounding of the
 * denominator eo_i + eo_j - ev_a - ev_b, whose value can depend on the order of a and b in the last bit).  Storage, shapes
 * and results otherwise as in the plain calls.  The forms run when pymes_sym_tail answers 1 — the o x o tile fits the LDS
 * (pymes_pair_fused_ok), the build has them, the environment does not say PYMES_SYM_TAIL=0 — and the call is too large to be
 * a task of a phase launch (PYMES_PHASE_MAX_US; small problems keep the plain forms whether phases are on or off, so that the
 * bits of a solve do not depend on the phase switches); otherwise they ARE the plain calls.  Not for EOM, Lambda or (T) vectors and not for the pair-compact arrays of the sharded loop.
 * pymes_dots_sym: sym[p] != 0 marks the pairs of symmetric [v,v,o,o] operands (n[p] = v*v*o*o), the others as pymes_dots_var.
 * pymes_diis_mix_sym: sym_types[t] != 0 marks the amplitude types whose vectors are such arrays.
 * pymes_pair_layouts_sym: pymes_pair_layouts (2 X_abij - X_baij with X_baij taken from the tile of X_ab).
 * Flag PYMES_SYM_TAIL of pymes_ccsd_residuals and pymes_doubles_residual (with PYMES_SYM_RINGS): the same declaration for
 * t2 — the pair layouts inside are formed that way; pymes_ccsd_iterate declares all of it itself. */
#define PYMES_SYM_TAIL (1u << 22)
int pymes_sym_tail(pymes_ctx* ctx, int* yes);
int pymes_cc_update_to_sym(pymes_ctx* ctx, double* t_out_dev, double* dt_dev, const double* t_in_dev, const double* r_dev,
                           double level_shift, double delta);                       /* rank 4; t_out may be t_in */
int pymes_dots_sym(pymes_ctx* ctx, int npairs, const double* const* x_dev, const double* const* y_dev, const int64_t* n,
                   const int* sym, double* out_host);
int pymes_lincomb_sym(pymes_ctx* ctx, double* out_dev, int nx, const double* const* x_dev, const double* c_host, int64_t n);
int pymes_diis_mix_sym(pymes_ctx* ctx, double* state_host, int ntypes, int m, int was_full, const double* const* err_hist_dev,
                       const double* const* err_new_dev, const int64_t* sizes, const double* const* amp_hist_dev,
                       double* const* out_dev, const int* sym_types);
int pymes_energy_norms_start_sym(pymes_ctx* ctx, const double* f_dev, const double* t1_dev, const double* t2_dev,
                                 const double* dt2_dev, int* slot);
int pymes_pair_layouts_sym(pymes_ctx* ctx, const double* x_dev, double* Xd_dev, double* Xx_dev, double* Xt_dev);
/* (yr + i yi)[e] = (mr + i mi)[e] (xr + i xi)[e], e < n: a complex diagonal applied to a complex vector held as two real
 * arrays (y may alias x) — the preconditioner 1 / (z - diag + 0.01) of the FEAST linear solves, feast_eom_ccsd.py:342-343. */
int pymes_cmul(pymes_ctx* ctx, const double* mr_dev, const double* mi_dev, const double* xr_dev, const double* xi_dev,
               double* yr_dev, double* yi_dev, int64_t n);

/* pymes/mean_field/hf.py:14-18 from the context's device blocks: f = h + 2 V_piqi - V_piiq (i occupied); h, f [n,n] host */
int pymes_hf_fock_matrix(pymes_ctx* ctx, const double* h_host, double* f_host);

/* ---- FCIDUMP ingestion: pymes/util/fcidump.py:59-163 with a native text parser -------------------
 * Same semantics as the reference's reader (header by substring match, "value i j k l" -> p r q s, |value| < 1e-19
 * skipped, the three index-swap images restored but not the electron-exchange one, is_tc: only [q,p,s,r]; a body line
 * without exactly five fields is an error).
 *   pymes_fcidump_header:    NELEC, NORB (to size the context)
 *   pymes_fcidump_read_host: everything on the host, V[n,n,n,n] caller-allocated (the drop-in fcidump.read)
 *   pymes_fcidump_load:      e_core / eps[n] / h[n,n] on the host, V packed into the context's 16 device blocks like
 *                            pymes_set_V_pqrs; for NORB > 64 the lines are uploaded in chunks and V_pqrs is filled on
 *                            the device (it never exists on the host; files whose symmetry-related lines disagree are
 *                            refused there because the result would depend on the order of the lines). */
int pymes_fcidump_header(const char* path, int* n_elec, int* n_orb);
int pymes_fcidump_read_host(const char* path, int is_tc, double* e_core, double* eps_host, double* h_host,
                            double* V_host);
int pymes_fcidump_load(pymes_ctx* ctx, const char* path, int is_tc, double* e_core, double* eps_host, double* h_host,
                       int64_t* n_two_electron_lines);

/* ---- packed binary integral files: the on-disk form of the 16 blocks (or of density-fitting factors) -------------
 * The reference has only text ingestion (fcidump.py:124-161, one Python iteration per line) plus the hdf5 branch of its
 * TCDUMP reader (tcdump.py:44-48,88-92).  Format "PYMESPK1" (pymes_amd/csrc/packed.h): 64-byte header, eps[n], h[n,n],
 * then either the 16 partition.py blocks as raw little-endian fp64 (kind 1) or factors B[naux,n,n] with
 * V[p,q,r,s] = sum_Q B[Q,p,r] B[Q,q,s] (kind 2).
 *   pymes_packed_header:         kind, NELEC, NORB, naux (to size the context)
 *   pymes_packed_load:           e_core / eps[n] / h[n,n] on the host, the payload straight into the context's 16
 *                                device blocks (kind 1: streamed block by block; kind 2: formed by the MFMA GEMM)
 *   pymes_packed_write:          the context's 16 blocks + the caller's one-body data -> file (kind 1)
 *   pymes_packed_write_factors:  host factors -> file (kind 2) */
int pymes_packed_header(const char* path, int* kind, int* n_elec, int* n_orb, int* naux);
int pymes_packed_load(pymes_ctx* ctx, const char* path, double* e_core, double* eps_host, double* h_host);
int pymes_packed_write(pymes_ctx* ctx, const char* path, int n_elec, double e_core, const double* eps_host,
                       const double* h_host);
int pymes_packed_write_factors(const char* path, int n_elec, int n_orb, int naux, double e_core, const double* eps_host,
                               const double* h_host, const double* B_host);

/* ---- EOM-CCSD sigma build as ONE entry per step: pymes/solver/eom_ccsd.py:268-385 (update_singles + update_doubles) --------
 * The reference builds sigma = H-bar u term by term from 62 einsums per trial vector.  pymes_eom_sigma_prepare hoists every V.T
 * product that does not depend on the trial vector (once per solve: the (ov)^2 pair matrices, the o v^3 / o^3 v blocks,
 * the one-index dressings; ~10 amplitude-sized arrays held by the handle), pymes_eom_sigma_apply builds sigma for k trial
 * vectors — k >= 2 exchange-symmetric vectors stacked so that every shared operand is read once (the Davidson driver,
 * eom_ccsd.py:95-101), anything else vector by vector, complex trial vectors as two real ones (the operator is real).
 *   f_host      T1-dressed Fock matrix [n,n] (host; eom_ccsd.py:46: t_fock_dressed_pq)
 *   t2_dev      CCSD doubles [v,v,o,o] on the device; must stay alive and unchanged until pymes_eom_sigma_destroy
 *   dressed     != 0: read the context's T1-dressed blocks (pymes_ccsd_dress_V, all of eom_ccsd.py's ten), else the blocks as set
 *   u1_dev[z] [v,o], u2_dev[z] [v,v,o,o] in; s1_dev[z], s2_dev[z] out (device; may not alias the inputs)
 *   sym[z]      != 0: u2[z]_abij = u2[z]_baji is known to hold; sym == NULL: tested (one reduction + synchronisation per vector)
 *   flags       bit 0 V_abcd = V_badc, 1 T_abij = T_baji, 2 pair-packed hole-ladder terms, 3 fused pair kernels, 4 stacked build
 * pymes_eom_diagonals: eom_ccsd.py:169-198 (get_diag_singles) and :200-266 (get_diag_doubles) on the device, d1 [v,o],
 * d2 [v,v,o,o] (needs no handle).  A handle belongs to its context: destroy it before pymes_ctx_destroy. */
typedef struct pymes_eom pymes_eom;
int pymes_eom_sigma_prepare(pymes_ctx* ctx, const double* f_host, const double* t2_dev, int dressed, pymes_eom** out);
int pymes_eom_sigma_flags(pymes_eom* h, int* flags);
int pymes_eom_sigma_apply(pymes_eom* h, int k, const double* const* u1_dev, const double* const* u2_dev, const int* sym,
                          double* const* s1_dev, double* const* s2_dev);
int pymes_eom_diagonals(pymes_ctx* ctx, const double* f_host, const double* t2_dev, int dressed, double* d1_dev, double* d2_dev);
/* releases the engine's pooled scratch that is not in use (the temporaries / hoisted arrays of destroyed EOM handles) */
int pymes_scratch_trim(pymes_ctx* ctx);
int pymes_eom_sigma_destroy(pymes_eom* h);

/* ---- IP- and EA-EOM-CCSD: ionisation and attachment energies (closed shell, doublet final states, right eigenvectors) ----------
 * The operator is the EE sigma above restricted to the sector with one extra orbital x that interacts with nothing: with x a
 * virtual, u1[x,i] = r1[i], u2[x,b,i,j] = u2[b,x,j,i] = r2[i,j,b] gives the IP operator plus eps_x; with x an occupied,
 * u1[a,x] = r1[a], u2[a,b,x,j] = u2[b,a,j,x] = r2[a,b,j] gives the EA operator minus eps_x.  Eigenvalues: E(N-1) - E(N) (IP),
 * E(N+1) - E(N) (EA).  With f the T1-dressed Fock matrix, V the T1-dressed blocks, t = T2 [a,b,i,j] and
 *   L_oo[l,i] = f_li + (2 V_klcd - V_kldc) t_cdki,  L_vv[a,d] = f_ad - (2 V_klcd t_cakl - V_klcd t_ackl),  W_klij = V_klij + V_klcd t_cdij,
 *   M1 = V_iabj[k,a,c,i] + V_klcd (2 t_caki - t_acki),  M_C = V_kldc t_caki,  M_D = V_kldc t_acki,  U = V_iajb[k,a,i,c]  as [(a,i),(d,l)],
 *   PA = 2 M1 + M_D - 2 M_C - U,  PB = M_C - M1,  MDU = M_D - U,   rt = 2 r2 - (r2 with its first two indices exchanged):
 * IP, r1[i], r2[i,j,b]:
 *   s1[i]     = f_jb rt[i,j,b] - L_oo[k,i] r1[k] - V_ijka[j,k,i,b] rt[j,k,b]
 *   s2[i,j,b] = -L_oo[l,i] r2[l,j,b] - L_oo[l,j] r2[i,l,b] + L_vv[b,d] r2[i,j,d] + W_klij r2[k,l,b] + t_cbij Y_c + A[l,i,j,b] r1[l]
 *               + PA[(b,j),(d,l)] r2[i,l,d] + PB[(b,j),(d,l)] r2[l,i,d] + MDU[(b,i),(d,l)] r2[l,j,d] - (r1[l] V_iabc[l,b,c,d]) t_cdij
 *   Y_c = -V_lkcd rt[l,k,d],   A[l,i,j,b] = -2 V_ijak[k,l,c,i] t_cbkj + V_ijka[k,l,i,c] t_cbkj + V_ijak[k,l,d,i] t_bdkj
 *                                           + V_ijka[k,l,j,d] t_bdki - V_iajk[l,b,i,j] - f_lc t_cbij
 * EA, r1[a], r2[a,b,j]:
 *   s1[a]     = f_jb rt[a,b,j] + L_vv[a,b] r1[b] + V_iabc[j,a,b,c] rt[c,b,j]
 *   s2[a,b,j] = L_vv[a,d] r2[d,b,j] + L_vv[b,c] r2[a,c,j] - L_oo[k,j] r2[a,b,k] + V_abcd r2[c,d,j]
 *               + t_abkl (V_kldc r2[d,c,j] + V_ijka[l,k,j,d] r1[d]) - t_abkj (V_kldc rt[d,c,l] + f_kd r1[d])
 *               + PA[(b,j),(d,l)] r2[a,d,l] + PB[(b,j),(d,l)] r2[d,a,l] + MDU[(a,j),(d,l)] r2[d,b,l]
 *               + Q[k,a,c] (2 t_cbkj - t_bckj) - Q'[k,a,c] t_cbkj - Q'[k,b,c] t_ackj + V_abic[b,a,j,c] r1[c],
 *   Q[k,a,c] = V_iabc[k,a,c,d] r1[d],  Q'[k,a,c] = V_iabc[k,a,d,c] r1[d]
 * (the 7 + 32 terms per operator that the restriction of eom_ccsd.py:268-385 leaves, factorised).  The operator needs
 * V_pqrs = V_qpsr on the blocks it reads and T_abij = T_baji: pymes_ipea_sigma_prepare tests both once and refuses, naming the
 * missing symmetry.  Hermiticity is not needed (transcorrelated integrals).  Blocks read — IP: ijab iabj iajb ijka ijak iabc iajk
 * klij (no abcd: works on an integral-sharded context); EA: ijab iabj iajb ijka iabc abic abcd (refuses a sharded context).
 *   f_host   T1-dressed Fock matrix [n,n] (host);   t2_dev   CCSD doubles [v,v,o,o], alive and unchanged until _destroy
 *   dressed  != 0: read the context's T1-dressed blocks (pymes_ccsd_dress_V), else the blocks as set
 *   _flags       bit 0: kind, bit 1: dressed
 *   _apply       sigma of k trial vectors (device): s1[z] [n1], s2[z] [n2]; n1 = o, n2 = o o v (IP) / n1 = v, n2 = v v o (EA).
 *                All k vectors go through every product as one GEMM: each hoisted operand and integral block is read once
 *   _diagonals   d1 = -L_ii (IP) / L_aa (EA);  d2 = L_bb - L_ii - L_jj (IP) / L_aa + L_bb - L_jj (EA)
 *   _correction  n roots in one launch over flat vectors [r1 (n1) | zero pad | r2 (n2)] of len doubles, the doubles at off2, d in
 *                the same layout: q_n = (s_n - w_n r_n) / (w_n - d + shift) written (zero in the pad), norms_host[2 n] =
 *                |s_n - w_n r_n|^2, norms_host[2 n + 1] = |r_n|^2 (fixed summation order; ONE synchronisation)
 * Every entry refuses a context that records a launch graph and a missing block by name; a refusal leaves no allocation behind.
 * A handle dies with its context (pymes_ctx_destroy invalidates it; _destroy then frees its shell). */
#define PYMES_IPEA_IP 0
#define PYMES_IPEA_EA 1
typedef struct pymes_ipea pymes_ipea;
int pymes_ipea_sigma_prepare(pymes_ctx* ctx, const double* f_host, const double* t2_dev, int dressed, int kind, pymes_ipea** out);
int pymes_ipea_sigma_flags(pymes_ipea* h, int* flags);
int pymes_ipea_sigma_apply(pymes_ipea* h, int k, const double* const* r1_dev, const double* const* r2_dev, double* const* s1_dev,
                           double* const* s2_dev);
int pymes_ipea_sigma_diagonals(pymes_ipea* h, double* d1_dev, double* d2_dev);
int pymes_ipea_sigma_correction(pymes_ipea* h, int n, const double* const* s_dev, const double* const* r_dev, const double* w_host,
                                const double* d_dev, double shift, double* const* q_dev, int64_t off2, int64_t len,
                                double* norms_host);
int pymes_ipea_sigma_destroy(pymes_ipea* h);
/* ---- left IP / EA vectors, Dyson amplitudes and pole strengths ---------------------------------------------------
 * H is the operator of pymes_ipea_sigma_apply on the compact vectors (r1, r2), <x, y> the plain sum over both arrays.
 * pymes_ipea_sigma_apply_left: o_z = H^T l_z for k vectors, stacked like _apply.  With U1, R, Rx, Rt (and Rn for EA) the packed
 * operands of the right build and D, E, L, S1 its partial results (s2[x,y,w] = D[x,y,w] + E[y,x,w] + L[x,y,w], s1 = S1):
 *   dD = l2,  dE = l2 with its first two indices exchanged,  dL = l2,  dS1 = l1      (the packing of the left vector)
 *   every product  C += alpha A . B  of the right build with the trial-vector operand A:  dA += alpha dC . B, the same hoisted
 *   operand or integral block B read through the same view (V_iabc in place, the EA ladder ONE product over V_abcd for all k)
 *   o2[x,y,w] = dR[x,y,w] + dRx[y,x,w] + 2 dRt[x,y,w] - dRt[y,x,w] (+ dRn[x,y,w]),  o1 = dU1   (the adjoint of the packing)
 * Left eigenvectors H^T l_k = w_k l_k are normalised <l_j, r_k> = delta_jk by the caller.
 * Dyson amplitudes.  Take the EE transition densities of pymes_tdm1 for the problem with the extra orbital x, T and Lambda
 * zero in x.  b_p: the restriction to the sector (one copy: [x,b,i,j] -> [i,j,b] for IP, [a,b,x,j] -> [a,b,j] for EA) of
 * d(R1, R2)/df_xp (IP) or d(R1, R2)/df_px (EA);  e_q: ONE HALF of the functional r -> gammaR[q,x] (IP) / gammaR[x,q] (EA) on the
 * embedded exchange-symmetric vector;  psiL_k(p) = <l_k, b_p>,  psiR_k(q) = <e_q, r_k>.  Written out (t = T2, Yoo[k,i] = sum
 * lam2[a,b,i,j] t[a,b,k,j], Yvv[a,c] = sum lam2[a,b,i,j] t[c,b,i,j]):
 * IP, l1[i], l2[i,j,b], r1[i], r2[i,j,b]:
 *   psiL(i) = l1[i]                              psiL(a) = sum_i l1[i] t1[a,i] + sum l2[i,j,b] t[a,b,i,j]
 *   psiR(a) = sum_i lam1[a,i] r1[i] / 2 + sum lam2[a,b,i,j] r2[i,j,b]
 *   psiR(j) = r1[j] + sum lam1[a,i] (2 r2[j,i,a] - r2[i,j,a]) / 2 - sum_i Yoo[j,i] r1[i] - sum_a t1[a,j] psiR(a)
 *   i.e. b_i = the unit single i,  b_a = (t1[a,:], t[a,b,i,j])
 * EA, l1[a], l2[a,b,j], r1[a], r2[a,b,j]:
 *   psiL(a) = l1[a]                              psiL(k) = -sum_a t1[a,k] l1[a] - sum l2[a,b,j] t[a,b,k,j]
 *   psiR(i) = -sum_a r1[a] lam1[a,i] / 2 - sum lam2[a,b,i,j] r2[a,b,j]
 *   psiR(b) = r1[b] + sum lam1[a,i] (2 r2[b,a,i] - r2[a,b,i]) / 2 - sum_a r1[a] Yvv[a,b] + sum_i psiR(i) t1[b,i]
 *   i.e. b_a = the unit single a,  b_k = -(t1[:,k], t[a,b,k,j])
 * Residue Z_k[q,p] = psiR_k(q) psiL_k(p), pole strength P_k = sum_p psiR_k(p) psiL_k(p); with V = 0 every Koopmans root has
 * P = 1.  Sum rules (identities in t, lambda): sum_c e_q[c] b_p[c] = rdm1[q,p] / 2 (IP), delta_qp - rdm1[p,q] / 2 (EA).
 * pymes_ipea_dyson: psiL_host, psiR_host [k,n] (occupied orbitals first) for k roots given as device vectors of the handle's
 * kind; t2 is the handle's.  Yoo, Yvv are built once per call, the root-dependent contractions are engine products with the k
 * vectors stacked, the rest one assembly launch.  Linear in every vector; reads no integral block; identical calls give
 * identical bits (no atomics, fixed summation order).  Both entries refuse a context that is recording a launch graph. */
int pymes_ipea_sigma_apply_left(pymes_ipea* h, int k, const double* const* l1_dev, const double* const* l2_dev,
                                double* const* o1_dev, double* const* o2_dev);
int pymes_ipea_dyson(pymes_ipea* h, const double* t1_dev, const double* lam1_dev, const double* lam2_dev, int k,
                     const double* const* l1_dev, const double* const* l2_dev, const double* const* r1_dev,
                     const double* const* r2_dev, double* psiL_host, double* psiR_host);
/* ---- CCSD Lambda equations and the one-particle density -----------------------------------------------------
 * Vectors are pairs (x1 [v,o], x2 [v,v,o,o]) with x2_abij = x2_baji; <x, y> is the plain sum over all elements of both arrays.
 * A is the EE-EOM-CCSD sigma of pymes_eom_sigma_apply (eom_ccsd.py:268-385), f~ / V the dressed Fock matrix and blocks of the
 * handle, t = T2.
 *   left sigma  A^T: <A^T l, u> = <l, A u> for all exchange-symmetric u, l.  Term by term it is the table of the sigma build
 *               with the trial vector and the output swapped: a row  c . einsum("X,Y,U->S", x, y, u)  becomes
 *               c . einsum("X,Y,S->U", x, y, l');  l' = l2 + l2^T(baji) for the rows under P(ijab,jiba) (:332-373), l2 for the
 *               four unpermuted ones (:380-383), l1 for the singles rows; the doubles result is symmetrised, (x + x^T(baji)) / 2.
 *               The hoisted V.T intermediates of the handle are read through transposed views; the particle ladder adjoint
 *               sum_ab V_abcd l2_abij runs pair-packed on the rows V+ / V- of the right build read transposed ((V^T)+- =
 *               (V+-)^T whenever V_abcd = V_badc: no hermiticity needed, dressed and transcorrelated blocks included).
 *   Lambda      eta1[a,i] = 2 f~_ov[i,a],  eta2[a,b,i,j] = 2 V_ijab[i,j,a,b] - V_ijab[i,j,b,a];  A^T lambda + eta = 0.
 *               pymes_lambda_step: res = eta + A^T lam;  out = lam - res / d;  err = -err_scale res / d;  *norm_host = |res|;
 *               d1 = eps_v[a] - eps_o[i] - shift,  d2 = eps_v[a] + eps_v[b] - eps_o[i] - eps_o[j] - shift  (the denominators
 *               of the CCSD update with their sign turned).  err is the error vector for a DIIS mixer: pymes_diis_step tests
 *               linear dependence with an ABSOLUTE 1e-12 on the overlaps, which plain updates pass below |res| ~ 1e-6; a
 *               fixed err_scale (the Python driver: 1e5) keeps the extrapolation alive down to |res| ~ 1e-11.  start != 0: lam is taken as zero and not read (it may be NULL), out = -eta / d.
 *               sym != 0: the caller knows that lam2 has the exchange symmetry (else tested: one more synchronisation).
 *   density     L(f) = E(f) + <lam1, R1(f)> + <lam2, R2(f)> with the CCSD energy expression and residuals at (t1, t2) is
 *               linear in the Fock matrix; gamma_pq = dL / df_pq (occupied orbitals first, not symmetric):
 *                 Xvv[a,c] = sum l2[a,b,i,j] t[c,b,i,j],  Xoo[k,i] = sum l2[a,b,i,j] t[a,b,k,j],
 *                 Xov[j,b] = sum l1[a,i] (2 t[a,b,i,j] - t[a,b,j,i])
 *                 gamma_vo[a,i] = l1[a,i]                      gamma_oo[j,i] = -2 Xoo[j,i] - sum_a t1[a,j] l1[a,i]
 *                 gamma_vv[a,b] = 2 Xvv[a,b] + sum_i l1[a,i] t1[b,i]
 *                 gamma_ov[j,b] = Xov[j,b] + 2 t1[b,j] + sum_i gamma_oo[j,i] t1[b,i] - 2 sum_a t1[a,j] Xvv[a,b]
 *               pymes_rdm1 writes gamma + ref on the occupied diagonal (ref = 2: the trace is the electron count) to
 *               gamma_host [n,n]; it reads no integral block.
 * All three refuse a context that is recording a launch graph; the first two refuse left doubles without the exchange
 * symmetry and (through the handle's prepare) an integral-sharded context and a missing block, by name.  Identical calls
 * give identical bits (no atomics, fixed summation order). */
int pymes_eom_sigma_apply_left(pymes_eom* h, int k, const double* const* l1_dev, const double* const* l2_dev, const int* sym,
                               double* const* o1_dev, double* const* o2_dev);
int pymes_lambda_step(pymes_eom* h, const double* lam1_dev, const double* lam2_dev, const double* eps_o_host,
                      const double* eps_v_host, double shift, double err_scale, int start, int sym, double* out1_dev, double* out2_dev,
                      double* err1_dev, double* err2_dev, double* norm_host);
int pymes_rdm1(pymes_ctx* ctx, const double* t1_dev, const double* t2_dev, const double* lam1_dev, const double* lam2_dev,
               double ref, double* gamma_host);
/* ---- the two-particle response density ---------------------------------------------------------------------------
 * L(f, V) = E(f, V) + <lam1, R1(f, V)> + <lam2, R2(f, V)> of the block above with the integrals switched on is linear and
 * homogeneous in (f, V).  G_pqrs = dL / dV_pqrs (f held fixed, all n^4 entries of V independent) and
 *   Gamma_pqrs = (G_pqrs + G_qpsr) / 2:   L(f, V) = sum gamma_pq f_pq + sum Gamma_pqrs V_pqrs  for every V with V_pqrs = V_qpsr
 * (gamma without the reference term; no factor 1/2; not hermitian and not symmetrised: V_pqrs = V_rspq is never assumed).  A
 * formula in (t1, t2, lam1, lam2): they need not solve anything.  G is the sum of (t = T2, tt = 2 t - t^(ab), tau = t + t1 t1):
 *   1 the coefficients of the T1-dressed blocks in <lam2, R2>:
 *       abij: l2      klij: B[k,l,i,j] = sum l2[a,b,i,j] t[a,b,k,l]      abcd: sum_ij l2[a,b,i,j] t[c,d,i,j]
 *       iajb[k,a,i,c] = -2 sum l2[a,b,i,j] t[c,b,k,j] - 2 sum l2[b,a,i,j] t[b,c,k,j]      iabj[k,b,c,j] = 2 sum l2[a,b,i,j] tt[a,c,i,k]
 *       ijab[k,l,c,d] = sum B[k,l,i,j] t[c,d,i,j] + sum l2[a,b,i,j] t[a,d,k,j] t[c,b,i,l] + sum l2[a,b,i,j] tt[a,c,i,k] tt[d,b,l,j]
 *                       - sum gvv[a,d] tt[a,c,l,k] + sum goo[l,i] tt[d,c,i,k] + 2 sum l2[a,b,i,j] t[d,a,k,i] (t[b,c,l,j] - t[c,b,l,j])
 *       (gvv = 2 Xvv, goo = -2 Xoo of pymes_rdm1);
 *   2 their back-transformation, the adjoint of the T1 dressing: a virtual bra index a of a dressed block sends -t1[a,k] times its
 *     coefficient to the occupied source index k, an occupied ket index i sends +t1[c,i] times it to the virtual source c — index
 *     by index, every subset of the transformable positions once (the abcd coefficient enters as sum_ij l2 tau, never as a v^4
 *     array unless the abcd block itself is asked for);
 *   3 the dressed-Fock part: with C the response density gamma without the energy's 2 t1 and C' = C without Xov in its ov block,
 *       V[j,p,b,q] += 2 t1[b,j] C'[p,q],   V[j,p,q,b] -= t1[b,j] C[p,q],   V_iabj[j,a,b,i] += 2 t1[b,j] Xov[i,a]
 *     (the last one: the reference dresses f_ov[i,a] with V_iabj[j,a,b,i]);
 *   4 the direct terms: V_aibc[a,j,b,c] += l1[a,i] tt[b,c,i,j];  V_ijka[j,k,i,b] -= l1[a,i] tt[a,b,j,k];
 *       V_ijab[k,j,b,c] -= (sum_a l1[a,i] t1[a,k]) tt[b,c,i,j];  V_ijab[j,k,c,b] -= (sum_i l1[a,i] t1[c,i]) tt[a,b,j,k];
 *       V_ijab[i,j,a,b] += 2 tau[a,b,i,j] - tau[b,a,i,j]  (the energy).
 * The full spin-summed two-particle density of E = sum h D1 + 1/2 sum V D with f = h + sum_i (2 V_piqi - V_piiq) is
 *   D_pqrs = D_HF + 2 (gamma_pr n_qs + n_pr gamma_qs) - (gamma_ps n_qr + n_ps gamma_qr) + 2 Gamma_pqrs,
 *   D_HF = 4 n_pr n_qs - 2 n_ps n_qr,  n the unit matrix on the occupied block (the host helper full_rdm2 of the Python package).
 * pymes_rdm2: writes the blocks named in mask (bit = 8 p + 4 q + 2 r + s of the pattern, 1 for a virtual position: klij 0,
 * ijka 1, ijab 3, iajk 4, iajb 5, iabj 6, iabc 7, abij 12, abic 13, abcd 15) to out_dev[bit], device arrays of the block's
 * shape.  A block and its image under (pq,rs) -> (qp,sr) hold the same numbers (Gamma_aibc[a,i,b,c] = Gamma_iabc[i,a,c,b], ...):
 * the six images (ijak, aijk, aibj, aijb, aibc, abci) are refused by name.  It reads no integral block (an integral-sharded
 * context is served).  abcd (v^4 doubles) is built only when its bit is set.
 * pymes_rdm2_expectation: *value_host = sum Gamma_pqrs W_pqrs over all sixteen blocks for the operator W held as the context's
 * undressed blocks (pymes_set_V_*); W_pqrs = W_qpsr is tested and refused by name otherwise, as is an integral-sharded context.
 * The abcd density is never built: sum Gamma_abcd W_abcd = sum l2[a,b,i,j] (sum_cd W_abcd tau[c,d,i,j]) with the inner sum
 * through the pair-packed ladder on W's packed V+ / V- rows.
 * Both refuse, by name and before any allocation: nocc > PYMES_NOCC_MAX_LAMBDA, a launch graph being recorded, lam2 or t2 without
 * the exchange symmetry x_abij = x_baji, (pymes_rdm2) outputs that alias inputs or each other.  Identical calls give identical
 * bits (no atomics, fixed summation order). */
int pymes_rdm2(pymes_ctx* ctx, const double* t1_dev, const double* t2_dev, const double* lam1_dev, const double* lam2_dev,
               unsigned mask, double* const* out_dev);
int pymes_rdm2_expectation(pymes_ctx* ctx, const double* t1_dev, const double* t2_dev, const double* lam1_dev,
                           const double* lam2_dev, double* value_host);
/* ---- left EOM-CCSD eigenvectors and transition densities ------------------------------------------------------
 * Conventions of the block above.  For root k: A r_k = w_k r_k, A^T l_k = w_k l_k (pymes_eom_sigma_apply / _apply_left; with
 * k > 1 the left build sends all vectors through its large products as one GEMM each), <l_j, r_k> = delta_jk,
 * r0_k = -<lambda, r_k>; the left state has no reference component.  R1(f), R2(f): the CCSD residuals at (t1, t2) with the
 * integrals set to zero; A(f): the sigma with the T1-dressed f and all V blocks zero.  Everything is linear in f:
 *   gammaL_k[p,q] = d/df_pq ( <l1_k, R1(f)> + <l2_k, R2(f)> )
 *   gammaR_k[p,q] = d/df_pq ( 2 sum f~_ov[i,a] r1_k[a,i] + <lambda, A(f) r_k> + 2 sum lambda2[a,b,i,j] r1_k[a,i] R1(f)[b,j]
 *                             - <lambda, r_k> ( <lambda1, R1(f)> + <lambda2, R2(f)> ) )
 *   S_k(O) = (sum gammaL_k O) (sum gammaR_k O);  oscillator strength (2/3) w_k sum_x S_k(mu_x).
 * Written out, with C the coefficients of the dressed Fock matrix f~ and the dressing undone at the end (t = T2):
 *   X(l1, l2):  Xvv[a,c] = sum l2[a,b,i,j] t[c,b,i,j],  Xoo[k,i] = sum l2[a,b,i,j] t[a,b,k,j],
 *               Xov[j,b] = sum l1[a,i] (2 t[a,b,i,j] - t[a,b,j,i])
 *   left:   C_vo = l1,  C_oo = -2 Xoo(l),  C_vv = 2 Xvv(l),  C_ov = Xov(l)          (pymes_rdm1 without ref and without 2 t1)
 *   right:  s = <lambda, r>,  Y = X(lambda1, lambda2),  Z = X(lambda1, lambda2) with r2 in the place of t,
 *           Le[b,j] = 2 sum lambda2[a,b,i,j] r1[a,i],  Eov = Xov(Le)
 *           C_vo = Le - s lambda1
 *           C_oo[j,i] = -sum_a r1[a,j] lambda1[a,i] - 2 Zoo[j,i] + 2 s Yoo[j,i]
 *           C_vv[a,b] = sum_i lambda1[a,i] r1[b,i] + 2 Zvv[a,b] - 2 s Yvv[a,b]
 *           C_ov[j,b] = 2 r1[b,j] + Zov[j,b] + Eov[j,b] - s Yov[j,b] - 2 sum_i Yoo[j,i] r1[b,i] - 2 sum_a Yvv[a,b] r1[a,j]
 *   gamma_vo = C_vo,  gamma_oo[j,i] = C_oo[j,i] - sum_a t1[a,j] C_vo[a,i],  gamma_vv[a,b] = C_vv[a,b] + sum_i C_vo[a,i] t1[b,i],
 *   gamma_ov[j,b] = C_ov[j,b] + sum_i gamma_oo[j,i] t1[b,i] - sum_a t1[a,j] C_vv[a,b]
 * pymes_tdm1: gammaL_host, gammaR_host [k,n,n] (occupied orbitals first) and r0_host [k] for k <= 64 roots given as device
 * vectors (l1[z], l2[z]), (r1[z], r2[z]); linear in every vector (the biorthogonal normalisation is the caller's).  The
 * contracted intermediates are engine products with the k vectors stacked, the rest one assembly launch.  It reads no integral
 * block; identical calls give identical bits (no atomics, fixed summation order).
 * pymes_eom_correction: the Davidson correction of pymes_ipea_sigma_correction for the EE vectors of the context's (no, nv):
 * flat vectors [x1 (v o) | zero pad | x2 (v v o o)] of len doubles, the doubles at off2, d_dev the diagonals of
 * pymes_eom_diagonals in the same layout (the same kernel; one launch and ONE synchronisation per sixteen roots).
 * Both refuse a context that is recording a launch graph. */
int pymes_tdm1(pymes_ctx* ctx, const double* t1_dev, const double* t2_dev, const double* lam1_dev, const double* lam2_dev, int k,
               const double* const* l1_dev, const double* const* l2_dev, const double* const* r1_dev, const double* const* r2_dev,
               double* gammaL_host, double* gammaR_host, double* r0_host);
int pymes_eom_correction(pymes_ctx* ctx, int n, const double* const* s_dev, const double* const* r_dev, const double* w_host,
                         const double* d_dev, double shift, double* const* q_dev, int64_t off2, int64_t len, double* norms_host);
/* ---- EOM-CCSD linear response functions ---------------------------------------------------------------------------
 * <<X;Y>>_z = sum_k [ <0|X|k><k|Y|0> / (z - w_k) - <0|Y|k><k|X|0> / (z + w_k) ] in its resolvent form, consistent with S_k(O) of
 * the block above (plain inner product, exchange-symmetric doubles, t = T2).  O~: the T1-dressed one-body operator,
 *   O~_ov[j,b] = O_ov,  O~_oo[j,i] = O_oo + O_ov t1,  O~_vv[a,b] = O_vv - t1 O_ov,  O~_vo[a,i] = O_vo + O_vv t1 - t1 O~_oo.
 * Right property vector xi(O) = (R1(O), R2(O)): the CCSD residuals at (t1, t2) with all integrals zero and f = O, so that
 * <l, xi(O)> = sum gammaL(l) O.  Written out:
 *   xi1[a,i] = O~_vo[a,i] + sum_jb (2 t[a,b,i,j] - t[a,b,j,i]) O~_ov[j,b]
 *   xi2 = S + S^T(1,0,3,2),  S[a,b,i,j] = sum_c O~_vv[a,c] t[c,b,i,j] - sum_k O~_oo[k,i] t[a,b,k,j]
 * Left property vector eta(O): <eta(O), r> = sum_pq gammaR(r)[p,q] O[p,q] for every exchange-symmetric r, gammaR the right
 * transition density above.  With Y = X(lambda1, lambda2) and g0 = <lambda, xi(O)>:
 *   eta1[c,k] = 2 O~_ov[k,c] + 2 sum_ai lambda2[c,a,k,i] xi1[a,i] - sum_i lambda1[c,i] O~_oo[k,i] + sum_a O~_vv[a,c] lambda1[a,k]
 *               - 2 sum_j Yoo[j,k] O~_ov[j,c] - 2 sum_b Yvv[c,b] O~_ov[k,b] - g0 lambda1[c,k]
 *   eta2 = (E + E^T(1,0,3,2)) / 2 - g0 lambda2,  E[a,b,i,j] = -2 sum_k lambda2[a,b,k,j] O~_oo[i,k] + 2 sum_c O~_vv[c,a] lambda2[c,b,i,j]
 *                                                            + 2 lambda1[a,i] O~_ov[j,b] - lambda1[a,j] O~_ov[i,b]
 * x^O(z) = (z - A)^-1 xi(O) on the exchange-symmetric subspace (A: pymes_eom_sigma_apply);
 *   <<X;Y>>_z = <eta(X), x^Y(z)> + <eta(Y), x^X(-z)>,   polarizability = -<<X;Y>>_z,   z = w + i gamma.
 * Where a written-out formula and its definition disagree, the definition rules.
 * pymes_response_vectors: xi1[z], eta1[z] [v,o] and xi2[z], eta2[z] [v,v,o,o] (arrays of k device pointers) and g0_host [k] for
 * k <= 64 operators ops_host [k,n,n] (occupied orbitals first, undressed, need not be symmetric).  The intermediates contracted
 * over o v are engine products with the operators stacked; the singles and g0 are one launch; xi2 and eta2 one launch each of ONE
 * kernel, out_z = P(M_z T - N_z T + outer products) + s_z T for all operators, T read once per eight operators, nothing staged in
 * LDS (no cap on nocc).  It reads no integral block.  Identical calls give identical bits (no atomics, fixed summation order);
 * xi2 and eta2 are exchange-symmetric to the bit when t2 and lambda2 are.  Refused by name: null arguments, outputs that alias
 * inputs or each other, t2 or lambda2 without the exchange symmetry, a context that is recording a launch graph.
 * The linear solver's sweep over n systems (z_s - A) x_s = xi_s, flat vectors [x1 (v o) | zero pad | x2 (v v o o)] of len doubles
 * with the doubles at off2, real and imaginary parts as two device vectors (all imaginary pointers null and Im z = 0: a real
 * system).  p: the preconditioned direction, ap = A p as the sigma build left it, q = z p - ap formed on the fly; hp, hq: the
 * nh <= PYMES_RESPONSE_HIST stored directions with (z - A) hp_j = hq_j and orthonormal hq_j; <u, v> = sum conj(u) v.
 * pymes_response_dots: dots_host[s][2 j], [2 j + 1] = <hq_j, q> for j < nh, then <q, q> (two doubles, the second 0) and <q, r>;
 * PYMES_RESPONSE_DOTS doubles per system.
 * pymes_response_update, the linear-system counterpart of pymes_eom_correction — all systems in one launch and one pass:
 *   ph = (p - sum_j g_j hp_j) inv,  qh = (q - sum_j g_j hq_j) inv  (written over p and ap: the next stored pair),
 *   x += alpha ph,  r -= alpha qh,  pn = r / (z - d),  norms_host[s] = |r|^2,
 * d_dev the diagonals of pymes_eom_diagonals in the flat layout; where |z - d| < floor the real part of z - d is replaced by
 * floor with its sign kept.  p null: no step (pn and |r|^2 of the r given: the start of a solve).  Both entries cost one
 * synchronisation whatever n (results through the pinned read-back ring up to 128 doubles), sum in a fixed order, and refuse null
 * arguments, a flat layout that does not match (no, nv), systems that are half real and half complex, and a context that is
 * recording a launch graph. */
#define PYMES_RESPONSE_HIST 32
#define PYMES_RESPONSE_DOTS (2 * (PYMES_RESPONSE_HIST + 2))
typedef struct pymes_response_system {
    double* x[2]; double* r[2]; double* p[2]; double* ap[2]; double* pn[2];      /* [0] real, [1] imaginary part */
    const double* hp[PYMES_RESPONSE_HIST][2];
    const double* hq[PYMES_RESPONSE_HIST][2];
    double g[PYMES_RESPONSE_HIST][2];
    double alpha[2], z[2], inv;
    int nh;
} pymes_response_system;
int pymes_response_vectors(pymes_ctx* ctx, const double* t1_dev, const double* t2_dev, const double* lam1_dev, const double* lam2_dev,
                           int k, const double* ops_host, double* const* xi1_dev, double* const* xi2_dev, double* const* eta1_dev,
                           double* const* eta2_dev, double* g0_host);
int pymes_response_dots(pymes_ctx* ctx, int n, const pymes_response_system* sys_host, int64_t off2, int64_t len, double* dots_host);
int pymes_response_update(pymes_ctx* ctx, int n, const pymes_response_system* sys_host, const double* d_dev, double floor,
                          int64_t off2, int64_t len, double* norms_host);
/* (mr + i mi)[e] = 1 / ((zr + i zi) - (hr + i hi) d[e] + shift), e < n: the FEAST preconditioner 1 / (z - diag + 0.01)
 * (feast_eom_ccsd.py:342; hs = 1j dt for the real-time form :276-278) from the device-resident diagonal */
int pymes_cshift_inv(pymes_ctx* ctx, const double* d_dev, double zr, double zi, double hr, double hi, double shift,
                     double* mr_dev, double* mi_dev, int64_t n);

/* ---- explicit 3-body (transcorrelated) operator ---------------------------------------
 * pymes/util/tcdump.py:52-56: dense fill of L[nb]^6 from (flat index, value) pairs — the host parser hands over
 * unique targets (the last of duplicate entries, as the reference's sequential assignment keeps). */
int pymes_scatter(pymes_ctx* ctx, double* dst_dev, uint64_t dst_elements, const int64_t* index_host,
                  const double* value_host, int64_t n);
/* pymes/integral/contraction.py:17-39 get_single_contraction -> D[p,r,q,s] ([nb]^4 on the device),
 * :41-65 get_double_contraction -> S[p,q], :67-95 get_triple_contraction -> scalar.
 * L_dev is [nb]^6 in the chemists' order (or|ps|qt) that tcdump.read returns. */
int pymes_tc_single_contraction(pymes_ctx* ctx, const double* L_dev, int nb, int no, double* D_dev);
int pymes_tc_double_contraction(pymes_ctx* ctx, const double* L_dev, int nb, int no, double* S_dev);
int pymes_tc_triple_contraction(pymes_ctx* ctx, const double* L_dev, int nb, int no, double* t0_host);

/* ---- measurement --------------------------------------------------------------------- */
/* executed-work counters since the last reset: GEMM launches, executed GEMM flops
 * (2*M*N*K*batch), permutation launches, bytes moved by explicit permutations */
int pymes_stats(pymes_ctx* ctx, int reset, int64_t* gemm_calls, double* gemm_flops, int64_t* permute_calls,
                double* permute_bytes);
/* HIP-event timing of every fp64 GEMM call on the context's stream (off by default).  kernel_class 0 = all
 * calls, 1 = the calls that ran on the LDS-DMA 128x128 MFMA kernel (the o^3v^3 / ladder products);
 * kernel_launches counts GEMM kernel launches (a call whose last tiles are k-split launches twice). */
int pymes_prof_enable(pymes_ctx* ctx, int on);
int pymes_prof_reset(pymes_ctx* ctx);
int pymes_prof_query(pymes_ctx* ctx, int kernel_class, int64_t* calls, int64_t* kernel_launches, double* total_ms,
                     double* flops);

#ifdef __cplusplus
}
#endif
#endif /* PYMES_AMD_H */
