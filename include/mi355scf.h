/*
 * mi355scf.h -- C ABI of the MI355X (gfx950) SCF Fock-build engine.
 *
 * Drop-in boundary.  The reference has no native plugin ABI: its scripts call
 * the Python surface of pyscf / gpu4pyscf, which in turn bind C libraries (libcint / libcvhf /
 * gpu4pyscf's libgvhf_rys, libgdft) through ctypes.  Each entry point below names the reference call
 * site that triggers it and the upstream C routine it stands in for [MEM = un-vendored upstream,
 * named from memory, not present under /root/reference].
 *
 * Conventions: extern "C"; plain pointers and sizes; every function returns 0 on success and a
 * negative code on failure (text via mi_last_error()); no exceptions cross the ABI.  `atm`, `bas`,
 * `env` follow the libcint layout (atm[natm][6], bas[nbas][8], env[]) that a PySCF-shaped Mole already
 * holds; only nctr == 1 shells with l <= 3 are accepted.  Pointers named d_* are DEVICE pointers
 * (e.g. torch.Tensor.data_ptr()) on the context's device; everything else is host memory.  `stream` is
 * a hipStream_t passed as void* (NULL = default stream).  All matrices are row-major [nao][nao] FP64.
 * A context is bound to one GPU and is not thread-safe; use one context per device/process.
 */
#ifndef MI355SCF_H
#define MI355SCF_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mi_ctx mi_ctx;

/* Last error text of the calling thread. */
const char *mi_last_error(void);

/* ABI version of this header/library pair. */
int mi_abi_version(void);

/* Create / destroy an engine context for one molecule+basis on GPU `device_id`.
 * Replaces: gto.Mole.build() handing _atm/_bas/_env to libcint (templates/calculate_energy.py:89-101;
 * templates/optimize_geometry.py:48-54). */
int mi_ctx_create(const int32_t *atm, int natm, const int32_t *bas, int nbas, const double *env,
                  int nenv, int device_id, mi_ctx **out);
void mi_ctx_destroy(mi_ctx *ctx);
int mi_ctx_nao(const mi_ctx *ctx);

/* A destroyed context parks its (possibly ~100 GB) tile store for reuse by the next context on the same
 * device (geometry optimisation); hand-over buffers, task lists and the pool of small device buffers are kept per device
 * as well.  This frees all of them.  (The library expects ONE host thread per device at a time: a second context working on
 * the same device from another thread gets private scratch buffers, but parked blocks are shared.) */
void mi_release_cache(void);

/* Tunables (project-defined, no reference counterpart).  Unknown keys are an error.
 * Effective at the next mi_eri_prepare:
 *   "runmax"      tiles per J/K work item (0 = auto)
 *   "jk_waves"    0 = one wave per work item, longest first; N > 0 = N waves with equal-cost contiguous shares
 *   "tri_tiles"   1 = block-diagonal tiles store triangular rows (default), 0 = full rows
 *   "jk_cache_mb" MiB of tiles (the leading, longest work items; jk_waves = 0 only) read with the default cache policy when the
 *                 tensor exceeds the Infinity Cache and the stream is nontemporal (default 160, 0 = none)
 *   "ao_order", "ket_cluster"  tile AO order (1 = angular-momentum major, 0 = caller's) / ket order inside Schwarz clusters
 *   "xf_mfma_min" transform kernel: FP64-MFMA tiles for spherical blocks of at least this many elements
 *   "eri_tpq", "tpq_maxprim"  thread-per-quartet kernels for the low angular classes / their contraction-depth limit
 *   "tpq_min_tasks"  ... and the fewest quartets of a class pair that they take (default 32768; the gradient reads it at each
 *                 call).  Smaller class pairs run on the wave-per-quartet kernels; tests set 1 to put every class on them
 *   "omega"       > 0: the store holds long-range integrals (ij|erf(omega r12)/r12|kl) instead of (ij|kl) (range-separated
 *                 hybrids: CAM-B3LYP's K_LR).  Every evaluation path (Rys pair, fused, thread-per-quartet) uses theta = omega^2 /
 *                 (omega^2 + rho), rho = pq/(p+q): Rys argument theta x, roots u theta, prefactor sqrt(theta).  Screening keeps
 *                 the FULL-Coulomb Schwarz table (a valid bound: erf(omega r)/r and erfc(omega r)/r are both positive definite,
 *                 so (ab|erf|ab) <= (ab|ab)); the LR store therefore has the tiles and the size of the full one.  mi_build_jk
 *                 (K only: d_J = NULL), mi_build_jk_multi, mi_eri_unpack, mi_eri_read_quartet and mi_eri_get_stats work on it
 *                 unchanged; mi_grad_eri*, mi_df_build and mi_df_grad refuse a context with omega != 0.  0 (default): full Coulomb.
 * Immediate:
 *   "jk_nt"       nontemporal loads for the tile stream (1 = when the tensor exceeds the Infinity Cache, 2 = always, 0 = never)
 *   "jk_pipe"     half-tile software pipeline for full-row tiles (-1 auto)
 *   "jk_pair"     n_dm = 2: one pass with two waves per work item (-1 = for stores > 16 GB, 0 = one pass per density, 1 = always)
 *   "grad_dtol"   derivative quartets with q_ab q_cd max|G| below this are skipped (default 1e-13, 0 = Schwarz only)
 *   "grad_live"   1 (default): that test runs once per class pair and the derivative launches walk the compacted list of live
 *                 quartets; 0: every launch screens per wave
 *   "grad_rows", "grad_rows_min", "grad_rows_g32"  row gradient kernel for the mid / high classes (1 = on, default), for
 *                 derivative blocks of at least this many rows (20), two quartets per wave up to 64 rows (1)
 *   "df_batch_max"  mi_df_build / mi_df_grad (set on the orbital context): at most this many (bra pair, auxiliary shell) tasks per
 *                 pass of an angular class (0, default: a pass is limited only by the 32 Mi-double hand-over buffer).  The
 *                 integrals do not depend on it to the bit; tests use a small value to run the several-pass loop
 *   "vmat_xcd"    xc_vmat: XCD-aware workgroup order (1, default: the tiles of one split share an XCD's L2; 0: natural order)
 *   "vmat_wgs"    xc_vmat: workgroups aimed at by the split over the grid points (0 = 1024, two full rounds; -1 = round-1 formula)
 *   "sp2_direct"  planned purification, one launch per pass, N <= 320: 1 = sp2_direct_kernel (MFMA operands loaded straight into
 *                 registers from the columns of the symmetric X, no LDS staging), 0 = sp2_plan_kernel (default of a new context;
 *                 the SCF driver sets 1) */
int mi_set_option(mi_ctx *ctx, const char *key, double value);

/* One-electron integrals into device buffers (any of them may be NULL): overlap S, kinetic T, nuclear
 * attraction V, dipole d_dip[3][nao][nao] about `origin` (host double[3], NULL = zero).  One launch per angular
 * class of shell pairs; V is summed over the nuclei by FP64 atomics (last-bit run-to-run differences).
 * Replaces: libcint int1e_ovlp_sph / int1e_kin_sph / int1e_nuc_sph / int1e_r_sph [MEM], reached from
 * mf.kernel() -> get_ovlp/get_hcore (templates/calculate_energy.py:155,205) and mf.dip_moment
 * (templates/calculate_energy.py:253). */
int mi_int1e(mi_ctx *ctx, double *d_S, double *d_T, double *d_V, double *d_dip, const double *origin,
             void *stream);

/* Evaluate the Schwarz-screened symmetry-unique four-centre ERIs once with the Rys-quadrature kernels
 * and keep them resident in HBM as 8x8x8x8 AO tiles.  `tol` is the Schwarz threshold
 * (PySCF direct_scf_tol = 1e-13 [MEM]).  (rank, nranks) select this process's shard of the tile runs
 * (SURVEY.md section 8e); pass (0, 1) for a single GPU.
 * Replaces: libcint int2e_sph + libcvhf CVHFnr_int2e_q_cond [MEM] / gpu4pyscf libgvhf_rys [MEM],
 * reached from mf.kernel() -> get_jk (templates/calculate_energy.py:155; optimize_geometry.py:90). */
int mi_eri_prepare(mi_ctx *ctx, double tol, int rank, int nranks, void *stream);
/* mi_eri_prepare returns MI_ERR_NOMEM (instead of -1) when this rank's share of the tile store does not fit in free HBM;
 * the caller then shards over more GPUs or falls back to the direct mode.  mi_eri_get_memory reports the bytes the last
 * mi_eri_prepare needed and the free HBM it saw (valid after success and after MI_ERR_NOMEM). */
#define MI_ERR_NOMEM (-2)
int mi_eri_get_memory(const mi_ctx *ctx, int64_t *need_bytes, int64_t *free_bytes);
/* Drop the resident store of the last mi_eri_prepare (parked for reuse by the next one).  A sharded run whose ranks agree on
 * the direct mode (because SOME rank's shard did not fit) calls this on the ranks whose shard did fit. */
int mi_eri_release(mi_ctx *ctx);
/* Fresh device allocations of tile stores of at least `min_bytes` made by this process so far (re-use of the parked store of
 * a destroyed / released context does not count): every step of optimize(mf) (templates/optimize_geometry.py:99) should reuse
 * ONE allocation. */
int64_t mi_tile_store_allocations(int64_t min_bytes);

/* Sharding plan without a GPU or a context: the (J,K,L) tile runs that survive the block-pair Schwarz table
 * qblk[nblk(nblk+1)/2] (nblk = ceil(nao/8); entry I(I+1)/2+J = max Schwarz factor of the shell pairs touching AO blocks I,J)
 * are dealt to `nranks` ranks longest-processing-time first by streamed bytes -- the same plan mi_eri_prepare follows
 * ("deal cost-balanced batches").  Outputs: bytes and runs per rank. */
int mi_plan_shards(int nao, const double *qblk, double tol, int nranks, int64_t *bytes_per_rank, int64_t *runs_per_rank);

/* Density fitting (`mf.density_fit()`): three-index (ij|P) and two-index (P|Q) Coulomb
 * integrals over the auxiliary basis held by the context `aux` -- an ordinary context (mi_ctx_create on the auxiliary
 * atm/bas/env) whose LAST shell is the unit function (s primitive, exponent 0, coefficient sqrt(4 pi)).  Evaluated by the same
 * Rys kernels as the four-centre integrals ((ij|P 1) quartets).  d_int3c[nao][nao][naux], d_int2c[naux][naux], naux =
 * mi_ctx_nao(aux) - 1; either may be NULL.  Replaces libcint int3c2e_sph / int2c2e_sph behind pyscf.df [MEM]. */
int mi_df_build(mi_ctx *ctx, mi_ctx *aux, double *d_int3c, double *d_int2c, void *stream);

/* Nuclear gradient of the fitted two-electron energy: d_grad[natm][3] += sum_{ab,P} Z3[a][b][P] d(ab|P)/dX
 * + sum_{PQ} Z2[P][Q] d(P|Q)/dX, with the three-index density d_Z3[nao][nao][naux] (symmetric in ab) and the two-index density
 * d_Z2[naux][naux] (symmetric) formed by the caller from the fitted tensor (either may be NULL).  `aux` as in mi_df_build (same
 * atom list as ctx).  The derivative-integral batches are dealt round-robin to `nranks` callers (rank 0 of 1: everything);
 * the caller adds the partial gradients.  Replaces libcint int3c2e_ip1 / int3c2e_ip2 / int2c2e_ip1 behind
 * pyscf.df.grad.rhf.get_jk [MEM] (`mf.density_fit().nuc_grad_method()`; the reference never calls it). */
int mi_df_grad(mi_ctx *ctx, mi_ctx *aux, const double *d_Z3, const double *d_Z2, double *d_grad, int rank, int nranks, void *stream);

/* Schwarz factors of the last mi_eri_prepare: q[nbas][nbas] (host), q_ab = sqrt(max |(ab|ab)|), 0 for dropped pairs.
 * Replaces: libcvhf CVHFnr_int2e_q_cond [MEM]. */
int mi_schwarz_get(const mi_ctx *ctx, double *q);

/* Test/debug: one shell quartet (ish jsh|ksh lsh) read back from the resident tiles into host memory
 * out[2li+1][2lj+1][2lk+1][2ll+1]; 0 where Schwarz screening dropped the tile, NaN where the tile lives on another rank.
 * Lets the parity tests compare individual integrals with libcint-style int2e_sph shell blocks [MEM] (oracle: orc_eri_shell). */
int mi_eri_read_quartet(mi_ctx *ctx, int ish, int jsh, int ksh, int lsh, double *out);

/* Statistics of the resident ERI store. */
typedef struct {
    int64_t n_tiles;          /* tiles resident on this rank                                    */
    int64_t n_runs;           /* (J,K,L) runs                                                    */
    int64_t stored_bytes;     /* bytes of tile payload streamed per J/K build on this rank       */
    int64_t n_unique_eri;     /* symmetry-unique (i>=j,k>=l,ij>=kl) ERIs inside the resident tiles */
    int64_t n_quartets;       /* shell quartets evaluated                                       */
    double  seconds_eri;      /* wall time of the one-off ERI evaluation                        */
} mi_eri_stats;
int mi_eri_get_stats(const mi_ctx *ctx, mi_eri_stats *out);

/* Coulomb and exchange matrices from the resident ERIs for n_dm density matrices:
 *   J_ij = sum_kl (ij|kl) D_kl,   K_ik = sum_jl (ij|kl) D_jl.
 * d_D, d_J, d_K: [n_dm][nao][nao]; d_J or d_K may be NULL to skip that matrix.  On a sharded context
 * the result is this rank's partial sum; the caller all-reduces (RCCL) across ranks.
 * Replaces: libcvhf CVHFnr_direct_drv with CVHFnrs8_ji_s2kl / CVHFnrs8_li_s2kj [MEM] / gpu4pyscf
 * RYS_build_jk [MEM], reached from get_jk / get_veff inside mf.kernel(). */
int mi_build_jk(mi_ctx *ctx, const double *d_D, int n_dm, double *d_J, double *d_K, void *stream);

/* Read-only description of what mi_build_jk(ctx, d_D, n_dm, with_j ? d_J : NULL, with_k ? d_K : NULL) would run on the current
 * store and options (n_dm > 2 runs as n_dm builds of one density): a NUL-terminated line of space-separated key=value fields
 *   family=plain|kjlt|pipe|pair  nt=0|1  dpp=0|1  tri=0|1  waves=<launched waves or wave pairs>  segments=<J/K work items>
 *   n_jk_cached=<leading work items read with the default cache policy under nt=1>
 * taken from the very function the launch consults.  Launches nothing and touches no GPU state; error before mi_eri_prepare or
 * when `len` is too small (128 bytes suffice).  Project-defined (tests, tuning); no reference counterpart. */
int mi_jk_describe(const mi_ctx *ctx, int with_j, int with_k, int n_dm, char *buf, size_t len);

/* J and K of n_dm densities that are each symmetric or antisymmetric, with every resident tile read once per batch
 * (linear response: many trial densities against one store).  sym: host array [n_dm], sym[m] = +1 (symmetric: J and K) or
 * -1 (antisymmetric: K; J[m] is written as zero, J of an antisymmetric density vanishes).  d_D, d_J, d_K: [n_dm][nao][nao]
 * device arrays; either d_J or d_K may be NULL (J only: the exchange contractions are skipped).  Requests beyond the per-launch batch (option "jk_multi_batch": default 8, at most 16)
 * run as several launches.  Sharded contexts return this rank's partial sums, as mi_build_jk does. */
int mi_build_jk_multi(mi_ctx *ctx, const double *d_D, int n_dm, const int *sym, double *d_J, double *d_K, void *stream);

/* Dense [nao^4] copy of the resident ERIs (chemists' notation (ij|kl), all eight symmetry images) for post-SCF methods on
 * small molecules: `mp.MP2(mf).kernel()` in templates/calculate_interaction.py:116-120.  Unsharded contexts only. */
int mi_eri_unpack(mi_ctx *ctx, double *d_out, void *stream);

/* First quarter of the AO -> MO transformation straight from the resident tiles (post-SCF methods at any size the store
 * fits: `mp.MP2(mf).kernel()`, templates/calculate_energy.py:117-141, calculate_interaction.py:116-120):
 *   Y[o][p][q][r] = sum_s C[s][o] (s p|q r),  o < nb,
 * d_C: [nao][ldc] device (column o of row s at d_C[s * ldc + o], ldc >= nb), d_Y: [nb][nao][nao][nao] device, caller's AO order,
 * exactly symmetric in (q, r); screened-out tiles contribute zero.  One streaming pass over the store per
 * mi_eri_qtrans_batch() (= 8) columns, larger requests run as several passes.  Allocates a padded accumulator of
 * min(nb, batch) * (8 ceil(nao / 8) + 8)^3 doubles for the duration of the call and synchronises `stream` before returning.
 * Unsharded contexts only (error otherwise, and before mi_eri_prepare); a long-range ("omega") store is transformed as it is.
 * Stands in for the first step of pyscf.ao2mo's half transformation (AO2MOnr_e1_drv) [MEM]. */
int mi_eri_qtrans(mi_ctx *ctx, const double *d_C, int nb, int ldc, double *d_Y, void *stream);
int mi_eri_qtrans_batch(void);

/* Active-pair Coulomb operators straight from the resident tiles (the two-electron input of a CASSCF macro iteration,
 * `mcscf.CASSCF(mf, ncas, nelecas).kernel()` in templates/calculate_casscf.py):
 *   Jp[vw][p][q] = sum_rs (pq|rs) Ca[r][v] Ca[s][w],  v >= w packed as vw = v (v + 1) / 2 + w,  npair = ncas (ncas + 1) / 2,
 * d_Ca: [nao][ldc] device (column v of row r at d_Ca[r * ldc + v], ldc >= ncas, 1 <= ncas <= 16), d_Jp: [npair][nao][nao] device,
 * caller's AO order, exactly symmetric in (p, q); screened-out tiles contribute zero.  The pair densities are formed on the
 * chip from the coefficient rows, never read from memory; one streaming pass over the store per mi_eri_active_j_width() (= 32)
 * pairs.  Allocates a padded accumulator of 32 (8 ceil(nao / 8) + 8)^2 doubles for the duration of the call and synchronises
 * `stream` before returning.  Unsharded contexts only (error otherwise, and before mi_eri_prepare).  Project-defined; stands
 * in for the (pq|vw) class of pyscf.mcscf.mc_ao2mo [MEM]. */
int mi_eri_active_j(mi_ctx *ctx, const double *d_Ca, int ncas, int ldc, double *d_Jp, void *stream);
int mi_eri_active_j_width(void);

/* Time `reps` back-to-back launches of the J/K digestion kernel alone with HIP events on `stream`
 * and return the average milliseconds per launch (bench.py's roofline leg). */
int mi_time_jk_kernel(mi_ctx *ctx, const double *d_D, int reps, double *ms_per_launch, void *stream);
/* Same measurement for the J-only (with_k = 0: the pure-functional RKS build) or K-only kernel variant. */
int mi_time_jk_variant(mi_ctx *ctx, const double *d_D, int with_j, int with_k, int reps, double *ms_per_launch,
                       void *stream);

/* DIIS (Pulay) helpers on device: given F, D, S form e = S D F - F D S ... */
/* err = A - A^T written in place of nothing: d_err[nao*nao] = d_SDF - d_SDF^T (fused epilogue). */
int mi_diis_errvec(mi_ctx *ctx, const double *d_SDF, double *d_err, void *stream);
/* d_out = sum_i coef[i] * d_hist[i]  (hist: n matrices of nao*nao, contiguous). coef on host. */
int mi_diis_combine(mi_ctx *ctx, const double *d_hist, const double *coef, int n, double *d_out,
                    void *stream);
/* Gram matrix row: out[i] = <d_hist_e[i], d_e> for i < n (host output, synchronises `stream`). */
int mi_diis_dots(mi_ctx *ctx, const double *d_hist_e, const double *d_e, int n, double *out,
                 void *stream);
/* Same, result left on the device (d_out[n]), no synchronisation: lets the SCF step fetch the Gram row,
 * the energy and the gradient norm with ONE device-to-host copy. */
int mi_diis_dots_dev(mi_ctx *ctx, const double *d_hist_e, const double *d_e, int n, double *d_out,
                     void *stream);
/* Round 2: the Pulay solve itself on the device, so that a cycle's extrapolation needs no host round trip (scf.diis.CDIIS ->
 * lib.diis.DIIS.extrapolate: numpy.linalg.solve of the (m+1)x(m+1) B-matrix system).  d_part = the [m][16] partials
 * mi_diis_dots_dev just wrote for the error vector in history slot `slot`; d_B [space][space] is the device-resident Gram
 * matrix (row/column `slot` are replaced), d_coef[0..m) receives the coefficients (no extrapolation, c = e_slot, when the
 * system is singular).  mi_diis_combine_dev = mi_diis_combine with the coefficients read from device memory. */
int mi_diis_solve(mi_ctx *ctx, const double *d_part, int m, int slot, int space, double *d_B, double *d_coef, void *stream);
int mi_diis_combine_dev(mi_ctx *ctx, const double *d_hist, const double *d_coef, int n, double *d_out, void *stream);
/* The same two with an explicit vector length `len` (doubles per history entry) instead of nao^2: the stacked (F_alpha, F_beta)
 * pair of UHF / UKS (scf.diis.CDIIS on the spin-stacked Fock matrix, templates/calculate_bde.py:126-128) has len = 2 nao^2. */
int mi_diis_dots_dev_n(mi_ctx *ctx, const double *d_hist_e, const double *d_e, int n, int64_t len, double *d_out, void *stream);
int mi_diis_combine_dev_n(mi_ctx *ctx, const double *d_hist, const double *d_coef, int n, int64_t len, double *d_out, void *stream);


/* ---- density from the Fock matrix without diagonalisation (row a11) ----------------------------- */
/* SP2 purification (Niklasson 2002) in an orthonormal basis; the X*X products are the caller's DGEMMs.
 * mi_sp2_init: X0 = (emax*I - F)/(emax - emin) with Gershgorin bounds; d_work: >= 2*n doubles.
 * mi_sp2_update: given X and X2 = X*X writes {tr X, tr X2, X_next[n*n]} to d_out_with_traces, where
 * X_next = X2 if |tr X2 - n_occ| < |2 tr X - tr X2 - n_occ| else 2X - X2.
 * Stand in for the LAPACK eig inside PySCF's SCF.eig (templates/calculate_energy.py:155 -> kernel()). */
int mi_sp2_init(mi_ctx *ctx, const double *d_F, double *d_X, double *d_work, void *stream);
int mi_sp2_update(mi_ctx *ctx, double *d_X, const double *d_X2, double n_occ, double *d_out_with_traces,
                  void *stream);

/* Fused SP2 for N <= 512: one launch per step (X*X on v_mfma_f64_16x16x4_f64 + branch + update + traces).
 * d_X holds X0 (or a previous iterate), d_X2 receives X^2; d_work: 2*n*n doubles; d_tr: 64*(nit+2) doubles.
 * Runs one squaring pass plus `nit` update+square passes; *d_tr_out points at ceil(n/16) interleaved PARTIAL traces
 * {tr X, tr X^2} (device); their sums in index order are the traces -- fixed-order partial sums instead of atomics, so that
 * the replicated algebra of a sharded run is bit-identical on every rank (no control-scalar broadcast needed). */
int mi_sp2_iterate(mi_ctx *ctx, double *d_X, double *d_X2, int nit, double n_occ, int have_x2,
                   double *d_work, double *d_tr, double **d_tr_out, void *stream);
/* Same passes on two caller-owned [X | X2] buffers without the final copy; *d_res = the buffer holding the result. */
int mi_sp2_iterate_pingpong(mi_ctx *ctx, double *d_A, double *d_B, int nit, double n_occ, double *d_tr, double **d_tr_out,
                            double **d_res, void *stream);

/* Planned purification: the whole sequence of quadratics is fixed by the caller from bounds of the spectrum (outer) and of
 * the HOMO / LUMO (inner) -- see mi355scf/sp2plan.py.  coef[3*(nit+1)]: pass 0 forms X_0 = coef[1] F + coef[2] I from the
 * (orthonormal-basis) Fock matrix d_F, pass k applies X_k = coef[3k] X^2 + coef[3k+1] X + coef[3k+2] I.  Buffers and trace
 * of every pass as in mi_sp2_iterate_pingpong (the caller validates tr(X - X^2) and tr X of the last pass).  One matrix per
 * pass: d_A, d_B need n^2 doubles each, *d_res = the one that holds the result out_scale * X_nit (2 = closed-shell density
 * matrix in the orthonormal basis; 0 or 1 = the projector itself; X_nit^2 is not stored); the traces are those of the
 * unscaled X. */
int mi_sp2_iterate_planned(mi_ctx *ctx, const double *d_F, double *d_A, double *d_B, int nit, const double *coef, double out_scale,
                           double *d_tr, double **d_tr_out, double **d_res, void *stream);

/* Fused elementwise pieces of one SCF cycle (rows a11/a12: get_fock + energy_elec, orbital-gradient norm):
 * mi_fock_energy: F = h + J - kscale*K (+Vxc); d_part[b] = block b's share of sum D*(h + (J - kscale*K)/2).  d_K, d_Vxc may be NULL.
 * mi_commutator_norm: E = M - M^T; d_part[b] = block b's share of |E|_F^2.
 * d_part has mi_reduce_blocks(ctx) = ceil(nao^2/256) entries; the caller adds them in index order (deterministic). */
int mi_reduce_blocks(const mi_ctx *ctx);
int mi_fock_energy(mi_ctx *ctx, const double *d_h, const double *d_J, const double *d_K, const double *d_Vxc,
                   const double *d_D, double kscale, double *d_F, double *d_part, void *stream);
int mi_commutator_norm(mi_ctx *ctx, const double *d_M, double *d_E, double *d_part, void *stream);

/* ---- DFT -------------------------------------------------------------- */

/* Becke fuzzy-cell weights for `ng` atom-centred grid points: d_coords[ng][3] (Bohr), d_atom_of[ng]
 * (owning atom), d_vol[ng] (radial x angular volume element), d_adjust[natm][natm] (Treutler radius
 * adjustment a_ij, device) -> d_weights[ng].  Replaces libdft VXCgen_grid [MEM], reached from
 * dft.RKS(mol) -> Grids.build (templates/calculate_energy.py:148,163; optimize_geometry.py:72,86).
 * Sizes, here and in mi_eval_ao / mi_xc_rho / mi_xc_rho_mo (the convention of mi_xc_aow): ng == 0 returns 0 without a
 * launch and leaves the output untouched; ng < 0 is an error ("negative"). */
int mi_grid_becke(mi_ctx *ctx, const double *d_coords, const int32_t *d_atom_of, const double *d_vol,
                  int64_t ng, const double *d_adjust, double *d_weights, void *stream);

/* Grid-weight response of a quadrature sum_g w_g e_g: d_out[natm][3] += sum_g d_e[g] d_vol[g] d(P_o / sum_B P_B)(r_g; R)/dR_C,
 * the total derivative of the Becke partition of mi_grid_becke (same inputs) with every point moving rigidly with its parent
 * atom; d_e[ng] is the UNWEIGHTED energy density per point.  FP64, O(natm^2) per point, reproducible to the bit.  The three
 * derivatives of every pair sum to zero, so sum_C d_out[C] keeps its value.  A point on a nucleus takes a zero unit vector.
 * ng == 0: d_out is left untouched; ng < 0 is an error.  PySCF: grad.rks.get_vxc_full / grids_response_cc [MEM]. */
int mi_grid_becke_grad(mi_ctx *ctx, const double *d_coords, const int32_t *d_atom_of, const double *d_vol, const double *d_e,
                       int64_t ng, const double *d_adjust, double *d_out, void *stream);

/* AO values (deriv=0), +gradient (deriv=1), +second derivatives xx,xy,xz,yy,yz,zz (deriv=2, for the XC
 * nuclear gradient) on grid points: d_ao[(1|4|10)][nao][ng]; any other deriv is an error.
 * Replaces libdft GTOval_sph_deriv1 / gpu4pyscf GDFTeval_gto [MEM] (numint.eval_ao). */
int mi_eval_ao(mi_ctx *ctx, const double *d_coords, int64_t ng, int deriv, double *d_ao, void *stream);

/* rho and grad rho from d_C = D @ ao0 ([nao][ng]): d_rho[(1|4)][ng].  (numint.eval_rho [MEM]) */
int mi_xc_rho(mi_ctx *ctx, const double *d_ao, const double *d_C, int64_t ng, int deriv, double *d_rho,
              void *stream);
/* Round 2: the same from occupied-orbital values d_psi[(1|4)][nocc][ng] = Z^T ao of a factorised density D = Z Z^T
 * (numint.eval_rho2 [MEM], what PySCF uses when mo_coeff / mo_occ are known): rho = sum psi^2, grad rho = 2 sum psi grad psi,
 * and (d_tau non-null, deriv = 1) the kinetic-energy density tau = 1/2 sum |grad psi|^2 of the meta-GGAs. */
int mi_xc_rho_mo(mi_ctx *ctx, const double *d_psi, int nocc, int64_t ng, int deriv, double *d_rho, double *d_tau, void *stream);
/* Fock matrix and energy partial sums straight from the J/K accumulators (single rank, resident tiles; the matrices J and K are
 * never formed): d_F = d_h + J - kscale K (+ d_Vun + d_Vun^T when d_Vun, an UNsymmetrised XC matrix, is given); d_part as in
 * mi_fock_energy.  with_k = 0: Coulomb only.  Same kernels as mi_build_jk for the digestion.
 * Replaces (with mi_build_jk / mi_fock_energy): get_veff + get_fock of the SCF classes, reached from mf.kernel(),
 * templates/calculate_energy.py:205. */
int mi_build_fock(mi_ctx *ctx, const double *d_D, const double *d_h, const double *d_Vun, int with_k, double kscale, double *d_F,
                  double *d_part, void *stream);
/* Warm start of the low-rank factor of the projector (project-defined; no reference counterpart): d_G[n][nocc] =
 * good ? 0.05 d_G0 + scale d_Zt^T : d_G0, good = (all of d_Zt[nocc][n] finite) && *d_info == 0, scale = 1 / |row 0 of d_Zt|. */
int mi_nystrom_warm(mi_ctx *ctx, const double *d_Zt, const int *d_info, const double *d_G0, double *d_G, int nocc, int n,
                    void *stream);
/* d_Zt[nocc][n] = R^-1 d_W^T with d_M[nocc][nocc] = R R^T (lower Cholesky factor), d_W[n][nocc]; *d_info = 0 or the 1-based index
 * of the first bad pivot (then d_Zt is NaN).  nocc <= 64.  Stands in for torch.linalg.cholesky_ex + solve_triangular. */
int mi_nystrom_factor(mi_ctx *ctx, const double *d_M, const double *d_W, int n, int nocc, double *d_Zt, int *d_info, void *stream);
/* d_tail[q] += sum_g d_w[g] d_vq[g] for the non-NULL d_v0..d_v2 (quadrature sums N_elec, E_xc of one grid block), one launch,
 * fixed summation order.  Stands in for the numpy dots at the end of numint.nr_rks / nr_uks [MEM]. */
int mi_xc_tail(mi_ctx *ctx, const double *d_w, const double *d_v0, const double *d_v1, const double *d_v2, int64_t ng, double *d_tail,
               void *stream);
/* Both steps fused (psi never stored): d_Zp[nao][ldz] = Z with the orbital index fastest, zero-padded to ldz = a multiple of
 * 24 (deriv = 1) or 32 (deriv = 0) columns; d_ao as in mi_xc_rho. */
int mi_xc_rho_lowrank(mi_ctx *ctx, const double *d_ao, const double *d_Zp, int ldz, int64_t ng, int deriv, double *d_rho,
                      double *d_tau, void *stream);

/* Closed-shell XC energy density and potential on the grid.  kinds[]: 1 Slater, 2 B88, 3 VWN-RPA,
 * 4 VWN5, 5 LYP, 6 PBE-x, 7 PBE-c, 12 short-range B88 (needs its omega in params: the _p entry points) with weights coefs[].  Outputs (any may be NULL): d_exc[ng] energy
 * per volume; d_wv[(1|4)][ng] = {w*vrho/2, 2*w*vsigma*grad rho}; d_vrho, d_vsigma raw derivatives.
 * Replaces libxc (HYB_GGA_XC_B3LYP etc.) reached through mf.xc (templates/calculate_energy.py:149). */
int mi_xc_eval(const int32_t *kinds, const double *coefs, int nterms, const double *d_rho,
               const double *d_w, int64_t ng, int gga, double *d_exc, double *d_wv, double *d_vrho,
               double *d_vsigma, void *stream);
/* Spin-polarised form for UKS (reference call sites templates/calculate_bde.py:128,140,197,215): rho_s = [rho, grad rho]
 * of spin s; wv_s feed mi_xc_aow / mi_xc_vmat exactly like the closed-shell wv and give V_xc of spin s. */
int mi_xc_eval_spin(const int32_t *kinds, const double *coefs, int nterms, const double *d_rhoa, const double *d_rhob,
                    const double *d_w, int64_t ng, int gga, double *d_exc, double *d_wva, double *d_wvb, void *stream);
/* The two above with one runtime parameter per term, params[nterms] (NULL: none; mi_xc_eval / mi_xc_eval_spin pass NULL).
 * Kind 12 = short-range B88 of CAM-B3LYP, params[i] = omega > 0 (required): per spin channel e_s^B88 F(a_s), ITYH attenuation
 * (Iikura, Tsuneda, Yanai, Hirao 2001) with a_s = omega / (2 k_s), k_s = sqrt(9 pi / K_s) rho_s^(1/3), e_s^B88 = -1/2
 * rho_s^(4/3) K_s; F(a) in closed form below a = 4 and by its asymptotic series from there (the closed form cancels in FP64).
 * The spin form applies it per channel by spin scaling.  Other kinds ignore their parameter.  Every XC entry point checks its
 * terms the same way: at most 8, known ids, a meta-GGA id only in mi_xc_eval_mgga*, kind 12 only with its omega (so never in
 * an entry point without params); ng < 0 is an error and ng == 0 returns 0 without a launch. */
int mi_xc_eval_p(const int32_t *kinds, const double *coefs, const double *params, int nterms, const double *d_rho,
                 const double *d_w, int64_t ng, int gga, double *d_exc, double *d_wv, double *d_vrho, double *d_vsigma, void *stream);
int mi_xc_eval_spin_p(const int32_t *kinds, const double *coefs, const double *params, int nterms, const double *d_rhoa,
                      const double *d_rhob, const double *d_w, int64_t ng, int gga, double *d_exc, double *d_wva, double *d_wvb,
                      void *stream);

/* XC response of closed-shell TDDFT, step 1: per point of the ground-state density d_rho[(1|4)][ng] (mi_xc_rho layout) the
 * weighted kernel coefficients d_coef[(1|4)][ng] = w {f_rr, f_rs, f_ss, v_s} (LDA, gga = 0: w f_rr only) of one response
 * channel, by second-order forward-mode dual numbers.  triplet = 0: second derivatives and v_sigma of the closed-shell
 * functional.  triplet = 1: the spin-difference combination of the spin-polarised functional at rho_a = rho_b = rho/2,
 * sigma_ss' = sigma/4: (f_aa - f_ab)/2, (f_a,saa - f_a,sbb)/4, (f_saa,saa - f_saa,sbb)/8, v_saa/2 - v_sab/4.  kinds / coefs /
 * params as mi_xc_eval_p (LDA and GGA kinds 1-7, 12; meta-GGA kinds are an error); points with rho <= 1e-10 get zero, the
 * cut-off of mi_xc_eval / mi_xc_eval_spin.  Replaces the fxc of libxc reached through pyscf.tdscf (numint.nr_rks_fxc /
 * nr_rks_fxc_st [MEM]). */
int mi_xc_fxc_prep(const int32_t *kinds, const double *coefs, const double *params, int nterms, const double *d_rho,
                   const double *d_w, int64_t ng, int gga, int triplet, double *d_coef, void *stream);
/* Step 2: m trial densities d_rho1[m][(1|4)][ng] (each from mi_xc_rho of a symmetric M) -> d_wv1[m][(1|4)][ng], the
 * linearised mi_xc_eval wv: with s1 = 2 grad rho0 . grad rho1, wv1[0] = 1/2 (c_rr rho1 + c_rs s1), wv1[1..3] =
 * 2 ((c_rs rho1 + c_ss s1) grad rho0 + c_s grad rho1), c = d_coef of step 1.  mi_xc_aow + mi_xc_vmat (or mi_xc_vmat_fold)
 * of each wv1[j] then give dV_xc[M_j] = vmat + vmat^T.  m == 0 or ng == 0: no-op. */
int mi_xc_fxc_apply(const double *d_rho0, const double *d_coef, const double *d_rho1, int m, int64_t ng, int gga, double *d_wv1,
                    void *stream);

/* d_aow[nao][ng] = sum_c d_ao[c] * d_wv[c]; Vxc = ao0 @ aow^T + transpose is then one DGEMM.  ng == 0: no-op. */
int mi_xc_aow(mi_ctx *ctx, const double *d_ao, const double *d_wv, int64_t ng, int gga, double *d_aow,
              void *stream);

/* ---- analytic nuclear gradient ---------------------------------------------- */
/* d_grad[natm][3] += 2 sum D <d mu|T+V|nu> - 2 sum W <d mu|nu> + Hellmann-Feynman terms.  d_W is the
 * energy-weighted density (D F D / 2).  One launch per angular class of ordered shell pairs.  Replaces libcint int1e_ipovlp/ipkin/ipnuc/iprinv [MEM], reached
 * through optimize(mf) -> mf.nuc_grad_method() (templates/optimize_geometry.py:99). */
int mi_grad_1e(mi_ctx *ctx, const double *d_D, const double *d_W, double *d_grad, void *stream);

/* d_grad[natm][3] += dE2/dR at fixed density: 2 sum (d mu nu|lam sig) [D D - hyb/4 (D D + D D)] over the
 * Schwarz-surviving quartets, derivative ERIs by the same Rys kernel on (l+1)/(l-1) auxiliary shells.
 * Replaces libcint int2e_ip1 + libcvhf nrs2/nrs4 J/K gradient contractions / gpu4pyscf rys gradient
 * kernels [MEM] (mf.nuc_grad_method().get_jk).  On a sharded context the quartet batches are dealt
 * round-robin to ranks: the result is a partial sum to be all-reduced by the caller.  Refused (error) on a context with
 * "omega" != 0: there are no long-range derivative integrals. */
int mi_grad_eri(mi_ctx *ctx, const double *d_D, double hyb, double *d_grad, void *stream);
/* Open-shell form (UHF/UKS, templates/calculate_bde.py:224 optimises radicals): d_D = Da + Db, d_Dspin = Da - Db
 * (NULL: closed shell); the exchange part contracts sum_s Ds x Ds = (D x D + M x M) / 2. */
int mi_grad_eri_spin(mi_ctx *ctx, const double *d_D, const double *d_Dspin, double hyb, double *d_grad, void *stream);
/* Same with the share of the derivative-quartet batches given explicitly (the two entry points above use the
 * (rank, nranks) of the last mi_eri_prepare, which in direct mode is a tile GROUP index, not the process's rank). */
int mi_grad_eri_sharded(mi_ctx *ctx, const double *d_D, const double *d_Dspin, double hyb, double *d_grad, int rank,
                        int nranks, void *stream);
/* The same pass with an extra pair term in the two-particle density of every quartet,
 *   G_abcd = D_ab D_cd - hyb/4 (D_ac D_bd + D_ad D_bc) (+ spin term) + sum_k s_k Q^k_ab Q^k_cd,
 * i.e. the gradient of 1/2 D.J[D] - hyb/4 (D.K[D] + M.K[M]) + 1/2 sum_k s_k (Q^k|Q^k): d_Q[K][nao][nao] symmetric
 * matrices on the device, s[K] on the host (finite), 0 <= K <= 136.  The density-weighted screening bound gains
 * qmax_ab qmax_cd, qmax_ab = sqrt(sum_k |s_k| max_ab |Q^k|^2).  K = 0 is mi_grad_eri_sharded.  Used for the active-space
 * cumulant of a CASSCF wavefunction (mcscf.CASSCF.nuc_grad_method). */
int mi_grad_eri_pairs(mi_ctx *ctx, const double *d_D, const double *d_Dspin, double hyb, const double *d_Q, const double *s,
                      int K, double *d_grad, int rank, int nranks, void *stream);
/* The same pass with signed exchange-type terms as well: the gradient, at fixed matrices, of
 *   1/2 (D|D) - hyb/4 [tr(D K[D]) + tr(M K[M])] + 1/2 sum_k s_k (Q^k|Q^k) + sum_m t_m sum_ijkl (ik|jl) R^m_ij R^m_kl,
 * i.e. every quartet's two-particle density gains sum_m t_m (R^m_ac R^m_bd + R^m_ad R^m_bc).  d_R[Kx][nao][nao] on the
 * device, each matrix symmetric (sym[m] = +1) or antisymmetric (sym[m] = -1) as declared (not verified: a matrix that is
 * neither gives a wrong gradient); t[Kx] (finite, either sign) and sym[Kx] on the host; 0 <= Kx <= 8.  D, M, Q, s, K as in
 * mi_grad_eri_pairs.  The screening bound gains xmax_ac xmax_bd + xmax_ad xmax_bc, xmax_ab = sqrt(sum_m |t_m| max_ab |R^m|^2).
 * Kx = 0 is mi_grad_eri_pairs.  Refused on a context with "omega" != 0.  Used for the relaxed two-particle density of a
 * TDA/TDDFT excited state (tdscf.TDA.nuc_grad_method). */
int mi_grad_eri_xpairs(mi_ctx *ctx, const double *d_D, const double *d_Dspin, double hyb, const double *d_Q, const double *s,
                       int K, const double *d_R, const double *t, const int *sym, int Kx, double *d_grad, int rank, int nranks,
                       void *stream);

/* meta-GGA evaluation (functional ids 8 TPSS exchange, 9 TPSS correlation, 10 M06-2X exchange, 11 M06-2X correlation; ids
 * 1-7 may be mixed in; 12 is refused, there is no params argument): d_tau[ng] = 1/2 sum_i |grad phi_i|^2; d_wv[5][ng] as mi_xc_eval plus d_wv[4] = w/4 de/dtau (the caller
 * adds sum_k ao_k^T (wv4 ao_k) to the unsymmetrised V_xc).  `--method M06-2X` at templates/calculate_energy.py:263;
 * default functional of templates/calculate_bde.py:105.  Stands in for libxc MGGA_X/C_TPSS, HYB_MGGA_X_M06_2X, MGGA_C_M06_2X
 * [MEM]; the M06-2X parameter tables are entered from memory (unverified). */
int mi_xc_eval_mgga(const int32_t *kinds, const double *coefs, int nterms, const double *d_rho, const double *d_tau,
                    const double *d_w, int64_t ng, double *d_exc, double *d_wv, void *stream);
/* Spin-polarised form (UKS): per spin rho_s[4][ng], tau_s[ng] -> wv_s[5][ng]. */
int mi_xc_eval_mgga_spin(const int32_t *kinds, const double *coefs, int nterms, const double *d_rhoa, const double *d_rhob,
                         const double *d_taua, const double *d_taub, const double *d_w, int64_t ng, double *d_exc, double *d_wva,
                         double *d_wvb, void *stream);

/* d_vmat[nao][nao] += ao0 . aow^T over the grid block (split-K FP64 MFMA kernel; rocBLAS has no split-K for
 * this tiny-M,N / huge-K shape and runs it at < 1 TFLOP/s).  The caller symmetrises (Vxc = vmat + vmat^T).  ng == 0 (here and
 * in mi_xc_vmat_fold): d_vmat is left untouched; ng < 0 is an error. */
int mi_xc_vmat(mi_ctx *ctx, const double *d_ao0, const double *d_aow, int64_t ng, double *d_vmat, void *stream);
/* Round 3: the same accumulation with the weighted AOs formed on the fly from the AO values and the weights x potential that
 * mi_xc_aow would take (d_ao [1|4][nao][ng], d_wv [1|4][ng], gga = 0: LDA): d_vmat += ao_0 . (sum_c wv_c ao_c)^T.  Replaces the
 * mi_xc_aow + mi_xc_vmat pair of numint.nr_rks's `_scale_ao` + `ao.T @ aow` [MEM] for LDA / GGA functionals. */
int mi_xc_vmat_fold(mi_ctx *ctx, const double *d_ao, const double *d_wv, int64_t ng, int gga, double *d_vmat, void *stream);

/* Real-solid-harmonic coefficient table used by the kernels: out[ncart(l)][2l+1] (host). */
int mi_c2s_table(int l, double *out);

/* Rys roots/weights as evaluated by the device tables, for tests: roots[n], weights[n] (host). */
int mi_rys_roots_host(int nroots, double x, double *roots, double *weights);

/* ---- C-PCM implicit solvation (additions; ABI version unchanged) ----------------------------------------------------------
 * Surface points d_pts[npts][4] = (x, y, z, zeta) in Bohr; point blocks d_blk[nblk][3] = (first point, count 1..64, owning
 * atom), every block inside the point list.  The store B[npts][ld], ld even and >= nao (nao + 1) / 2, holds
 *   B[g][m (m + 1) / 2 + n] = int phi_m phi_n erf(zeta_g |r - s_g|) / |r - s_g| dr   (m >= n, caller's AO order; padding 0).
 * mi_pcm_eval:      B, once per geometry (Rys quadrature with the erf attenuation; one launch per angular class).
 * mi_pcm_potential: d_dpack[ld] = D packed (off-diagonals D_mn + D_nm), d_v[g] = d_vn[g] - (B d)[g] (d_vn NULL: + (B d)[g]);
 *                   one workgroup per row, fixed-order sums.
 * mi_pcm_fock:      d_V[nao][nao] (accumulate ? += : =) scale * sum_g q_g B[g] unpacked symmetric; d_part holds
 *                   mi_pcm_fock_chunks(npts, ld) * ld doubles of per-chunk column sums (added in index order, no atomics).
 * mi_pcm_pairs:     the shell pairs of the launches (ordered = 1: all (i, j), the gradient's rows); returns their number,
 *                   fills out[n][2] when out is not NULL.
 * mi_pcm_grad:      d_part[n_ordered_pairs][nblk][3] = -2 sum_{g in block} q_g sum_{m in i, n in j} D_mn <d_A m|erf/r|n>_g, d_A the
 *                   derivative with respect to the centre of shell i acting on the bra function m alone (also when j sits on
 *                   the same centre: the ket's derivative is the row (j, i)); D is read as given, not symmetrised.  The row is
 *                   the share of the atom of shell i; the block's owning atom takes minus it (translational invariance). */
int mi_pcm_pairs(mi_ctx *ctx, int ordered, int32_t *out);
int mi_pcm_eval(mi_ctx *ctx, const double *d_pts, int npts, const int32_t *d_blk, int nblk, int64_t ld, double *d_B, void *stream);
int mi_pcm_potential(mi_ctx *ctx, const double *d_B, int npts, int64_t ld, const double *d_D, double *d_dpack, const double *d_vn,
                     double *d_v, void *stream);
int mi_pcm_fock_chunks(int npts, int64_t ld);
int mi_pcm_fock(mi_ctx *ctx, const double *d_B, int npts, int64_t ld, const double *d_q, double scale, int accumulate, double *d_part,
                double *d_V, void *stream);
int mi_pcm_grad(mi_ctx *ctx, const double *d_pts, int npts, const int32_t *d_blk, int nblk, const double *d_D, const double *d_q,
                double *d_part, void *stream);

/* ---- point-charge embedding (additions; ABI version unchanged) --------------------------------------------------------------
 * Sites d_pts[npts][4] = (x, y, z, zeta) in Bohr with charges d_q[npts]: zeta <= 0 a point charge g(r) = 1/r, zeta > 0 a
 * Gaussian charge g(r) = erf(zeta r)/r (the C-PCM convention).  The integrals are formed, contracted and discarded in one pass:
 * no buffer of size pairs x points exists, every sum has a fixed order (no atomics; two calls give identical bits).  Null
 * arguments, npts < 0 and non-finite coordinates, widths or charges are refused; npts == 0 is a no-op (mi_pc_grad: zero d_grad_atoms).
 * mi_pc_fock:        d_V[nao][nao] (accumulate ? += : =) scale * sum_k q_k (m| g_k |n).  d_work holds
 *                    mi_pc_fock_chunks(npts, ld) * ld doubles with ld = nao (nao + 1) / 2 rounded up to even: one packed
 *                    partial matrix per chunk of points, added in index order.
 * mi_pc_fock_chunks: the number of point chunks, at most 64; chunk k holds the points [k per, (k + 1) per), per = 256 up to
 *                    16 384 points and ceil(npts / 64) rounded up to a multiple of 64 beyond (ld does not enter).
 * mi_pc_grad:        the derivative of sum_k q_k sum_mn D_mn (m| g_k |n), D symmetric, with respect to the basis centres,
 *                    d_grad_atoms[natm][3], and to the sites, d_grad_pts[npts][3] (minus the sum of the bra derivatives of the
 *                    ordered pairs: translational invariance).  d_work holds mi_pc_grad_work(ctx, npts) doubles:
 *                    [ordered pairs][site blocks][3] for the atoms (blocks of 64 sites, growing to 512 beyond 32 768 sites) and
 *                    [pair chunks][npts][3] for the sites (at most 1024 chunks and, beyond 5 461 sites, at most 128 MB).
 * Both entry points copy the sites to the host and synchronise the stream once per call (the finiteness check): they belong in
 * the per-geometry set-up, not in a captured graph. */
int mi_pc_fock_chunks(int npts, int64_t ld);
int mi_pc_fock(mi_ctx *ctx, const double *d_pts, const double *d_q, int npts, double scale, int accumulate, double *d_work, double *d_V,
               void *stream);
int64_t mi_pc_grad_work(mi_ctx *ctx, int npts);
int mi_pc_grad(mi_ctx *ctx, const double *d_pts, const double *d_q, int npts, const double *d_D, double *d_work, double *d_grad_atoms,
               double *d_grad_pts, void *stream);

/* ---- determinant full CI in an active space (additions; ABI version unchanged; no context: nothing depends on the molecule) ----
 * `mcscf.CASCI(mf, ncas, nelecas).kernel()` -> fcisolver.kernel (templates/calculate_casscf.py:126-131); stands in for
 * pyscf.fci.direct_spin1's FCIcontract_2e_spin1 / FCImake_hdiag_uhf / FCIrdm12kern_sf of libfci [MEM].
 * norb <= 16 orbitals; strings are occupation bit masks numbered in ascending integer order; the determinant |Ia Ib> is (alpha
 * creators ascending)(beta creators ascending)|0>; CI vectors d_c / d_sigma are [nvec][nsa][nsb], beta string fastest.
 * Link tables (mi355scf/fci.py builds them): a link a+_cre a_ann |J> = sgn |T> is the pair (ann * norb + cre, sgn * (T + 1));
 * d_alink[nsa][nla][2] lists the nla links of every alpha string, d_btab[norb^2][nsb] holds the beta links densely (0 = none).
 * Work arrays cover alpha rows [a0, a0 + nrow) of every vector: W[(plane * nvec + v) * (nrow * nsb) + (Ia - a0) * nsb + Ib],
 * norb^2 + 1 planes.
 * mi_fci_gather_d:     D[r * norb + s] = <J|E_rs|c_v> (mode 1: alpha part, 2: beta part, 3: spin-summed); D[norb^2] = c_v.
 * mi_fci_gather_sigma: d_sigma[v][I] += sum_pq sum_{K in rows} <I|E_pq|K> F[p * norb + q][v][K] for EVERY I (planes 0..norb^2-1
 *                      of F); the caller zeroes d_sigma and calls once per chunk of rows.  Gather only, no atomics.
 * mi_fci_hdiag:        d_out[Ia][Ib] = <Ia Ib|H|Ia Ib> from h1[norb][norb], jdiag[p][q] = (pp|qq), kdiag[p][q] = (pq|qp) and the
 *                      string masks d_astr[nsa], d_bstr[nsb]. */
int mi_fci_gather_d(const double *d_c, int nvec, int nsa, int nsb, int norb, int a0, int nrow, const int32_t *d_alink, int nla,
                    const int32_t *d_btab, int mode, double *d_D, void *stream);
int mi_fci_gather_sigma(const double *d_F, int nvec, int nsa, int nsb, int norb, int a0, int nrow, const int32_t *d_alink, int nla,
                        const int32_t *d_btab, double *d_sigma, void *stream);
int mi_fci_hdiag(const double *d_h1, const double *d_jdiag, const double *d_kdiag, int norb, const int32_t *d_astr, int nsa,
                 const int32_t *d_bstr, int nsb, double *d_out, void *stream);

/* Closed-shell coupled cluster (mi355scf/ccsd.py).  Context-free; all arrays FP64 on the device.
 * `cc.CCSD(mf).kernel()` / `.ccsd_t()` (reference README, "adding a new method").
 * mi_cc_amp_update: one pass over the stacked vector [t1 (nocc nvir) | t2 (nocc nocc nvir nvir, layout i j a b)] of a CCSD cycle:
 *                   d_tnew = d_num / D (D = e_i - e_a, e_i + e_j - e_a - e_b), d_err = d_tnew - d_told, d_out[0] = sum |d_err|^2,
 *                   d_out[1] = sum_ijab (t2 + t1 t1)(2 (ia|jb) - (ib|ja)) of the NEW amplitudes against d_ovov[i][a][j][b].  Sums are
 *                   per workgroup, then in workgroup order (d_part: 2 * mi_cc_amp_blocks() doubles of work space): bit-reproducible.
 * mi_cc_t_energy:   the (T) correction of `ntrip` occupied triples after the GEMMs.  d_raw[6][ntrip][nvir^3]: cube p of triple t is
 *                   X(pi_p(i, j, k)) in its own index order, pi_p the p-th permutation of three objects in lexicographic order and
 *                   X(i, j, k)[a][b][c] = sum_d (ia|bd) t2[k][j][c][d] - sum_l (ia|lj) t2[l][k][b][c].  d_ijk[ntrip][3], d_wt[ntrip] the
 *                   triple's weight, d_t1[nocc][nvir], d_ovov[i][a][j][b], d_eo / d_ev the orbital energies.  d_et[t] = d_wt[t] * sum_abc
 *                   (4 W_abc + W_bca + W_cab - 2 W_acb - 2 W_cba - 2 W_bac) V_abc / (3 D).  d_part: ntrip * mi_cc_t_blocks(nvir) doubles
 *                   of work space (one partial sum per workgroup, added in workgroup order: no atomics, bit-reproducible). */
int mi_cc_amp_blocks(void);
int mi_cc_amp_update(const double *d_num, const double *d_told, double *d_tnew, double *d_err, const double *d_ovov, const double *d_eo,
                     const double *d_ev, int nocc, int nvir, double *d_part, double *d_out, void *stream);
int mi_cc_t_blocks(int nvir);
int mi_cc_t_energy(const double *d_raw, int ntrip, int nvir, int nocc, const int32_t *d_ijk, const double *d_wt, const double *d_t1,
                   const double *d_ovov, const double *d_eo, const double *d_ev, double *d_part, double *d_et, void *stream);

/* Restricted open-shell SCF (mi355scf/rohf.py).  Context-free; all arrays FP64 on the device.
 * mi_rohf_fock: Roothaan's effective Fock operator from the alpha and beta Fock matrices in the current MO basis, d_fa / d_fb
 *               [nmo][ld] row-major (ld >= nmo).  Orbitals [0, ncore) are doubly occupied, [ncore, ncore + nopen) singly, the
 *               rest empty; with Fc = (Fa + Fb) / 2
 *                   d_feff[i][j] = Fb between closed and open, Fa between open and virtual, Fc everywhere else,
 *                   d_g[i][j]    = sgn(class(i) - class(j)) d_feff[i][j]    (class: closed 0, open 1, virtual 2; 0 inside a class),
 *               the ROHF orbital gradient with the sign pattern of F n - n F (the CDIIS error vector in the MO basis).  Both
 *               outputs are [nmo][ld]; elements j >= nmo of a row are not touched.  d_part: 2 * mi_rohf_fock_blocks() doubles,
 *               d_part[b] = partial sum of d_g^2 and d_part[mi_rohf_fock_blocks() + b] = partial max |d_g| of workgroup b (every
 *               entry is written; the caller adds / maximises them).  No atomics, one writer per element: bit-reproducible. */
int mi_rohf_fock_blocks(void);
int mi_rohf_fock(const double *d_fa, const double *d_fb, int64_t ld, int ncore, int nopen, int nmo, double *d_feff, double *d_g,
                 double *d_part, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355SCF_H */
