/*
 * cmtfpls.h -- C ABI of the MI355X (gfx950) NIPALS engine for tensor PLS / coupled tensor PLS.
 *
 * The reference (meyer-lab/cmtf-pls) has no FFI seam: its hot path is a chain of NumPy / tensorly
 * calls inside tPLS.fit (cmtf_pls/tpls.py:73-120) and ctPLS.fit (cmtf_pls/cmtf.py:85-140).  Each
 * entry point below replaces ONE of those call sites (cited per function) and is what a binding on
 * the reference side would call (INTEGRATION.md shows the ctypes stub).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer owned by the caller (e.g. a torch tensor's data_ptr());
 *   - X is C-order (I, P) where P is the product of all trailing modes: the mode-0 unfolding is a
 *     free view, every sweep reads contiguous rows;  X is stored as f32 or f64 (suffix), every
 *     other operand (scores, loadings, Y, sums) is f64;
 *   - trailing-mode loadings are passed as two vectors wA (length A) and wB (length B), A*B == P,
 *     meaning w[c] = wA[c / B] * wB[c % B]  (order-3 X: wA = w_J, wB = w_K; a matrix X: A = 1);
 *   - `stream` is a hipStream_t passed as void*; all work is asynchronous on it; nothing here
 *     allocates, synchronises or throws: scratch comes from the caller (`ws`, size from the
 *     matching *_workspace_bytes);
 *   - return value: 0 ok, 1 bad argument, 2 workspace too small, 3 HIP error, 4 unsupported shape.
 *   - missing values are NaNs stored in-band in X (they persist through deflation exactly as in
 *     the reference, where NaN - x = NaN).
 */
#ifndef CMTFPLS_H
#define CMTFPLS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CMTFPLS_OK 0
#define CMTFPLS_EINVAL 1
#define CMTFPLS_EWORKSPACE 2
#define CMTFPLS_EHIP 3
#define CMTFPLS_EUNSUPPORTED 4

int cmtfpls_abi_version(void);
const char* cmtfpls_last_error(void);
/* Reset the HIP runtime's per-thread last error and this library's message; returns 1 if an error was pending.  For callers
 * that capture launch sequences into HIP graphs: a capture that fails leaves the error set, and the next entry would report it. */
int cmtfpls_clear_error(void);
/* A few status words (convergence norm, rank-1 flags) to PINNED host memory behind the work enqueued so far, then `event`
 * (a hipEvent_t, nullable) recorded: what the host waits on once per NIPALS iteration (tpls.py:103-107) -- one call instead
 * of a framework copy + record, because the pipelined inner loop (engine.FitRun._inner_loop_xcov_pipelined) is bound by host time. */
int cmtfpls_status_to_host(const void* src, void* dst_host, size_t bytes, void* event, void* stream);

/* ---- preprocess: tpls.py:61-71, cmtf.py:74-83 ------------------------------------------------
 * colstats: colsum[c] = sum over non-NaN i of X[i,c]; colcnt[c] = number of non-NaN i
 *           (np.nanmean = colsum / colcnt; np.isnan mask counts).  ws >= colstats_workspace_bytes.
 * center:   X[i,c] -= mean[c] in place (NaN stays NaN); rowcnt[i] (nullable) = non-NaN count of
 *           row i; ssq_part (nullable, >= center_partials() doubles) = per-block partial sums of
 *           the squared centred observed entries (||X_c||^2, denominator of calcR2X util.py:14). */
size_t cmtfpls_colstats_workspace_bytes(int64_t I, int64_t P);
int cmtfpls_colstats_f32(const float* X, int64_t I, int64_t P, double* colsum, double* colcnt,
                         void* ws, size_t ws_bytes, void* stream);
int cmtfpls_colstats_f64(const double* X, int64_t I, int64_t P, double* colsum, double* colcnt,
                         void* ws, size_t ws_bytes, void* stream);
int cmtfpls_sweep_partials(void); /* number of doubles every *ssq_part* argument must hold */
int cmtfpls_center_f32(float* X, int64_t I, int64_t P, const double* mean, double* rowcnt,
                       double* ssq_part, void* stream);
int cmtfpls_center_f64(double* X, int64_t I, int64_t P, const double* mean, double* rowcnt,
                       double* ssq_part, void* stream);

/* ---- K1 mode-0 contraction: np.einsum("i...,i...->...", X, u)  tpls.py:83, cmtf.py:94 --------
 * Z[c] = sum_i X[i,c] * u[i]   (f64 accumulation, deterministic two-stage sum).
 * masked != 0: NaN entries contribute 0 (numerator of miss_tensordot, missingvals.py:19);
 * the I/n_obs rescale is cmtfpls_colscale_f64 so that it can follow a cross-GPU all-reduce. */
size_t cmtfpls_mode0_contract_workspace_bytes(int64_t I, int64_t P);
int cmtfpls_mode0_contract_f32(const float* X, int64_t I, int64_t P, const double* u, double* Z,
                               int masked, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_mode0_contract_f64(const double* X, int64_t I, int64_t P, const double* u, double* Z,
                               int masked, void* ws, size_t ws_bytes, void* stream);
/* The same contraction with u = Y q (tpls.py:102, `Y @ Y_load`) formed inside the kernel instead of
 * being read: Z[c] = sum_i X[i,c] * (Y[i,:] . q).  Saves the u = Y q launch of every iteration.
 * Vector shapes (P % (16/sizeof(T)) == 0) with M <= 64 only: CMTFPLS_EUNSUPPORTED otherwise (form u with
 * cmtfpls_rowdot_f64 and call cmtfpls_mode0_contract_*).  Same workspace as mode0_contract. */
int cmtfpls_mode0_contract_yq_f32(const float* X, int64_t I, int64_t P, const double* Y, int ldy, int M,
                                  const double* q, double* Z, int masked, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_mode0_contract_yq_f64(const double* X, int64_t I, int64_t P, const double* Y, int ldy, int M,
                                  const double* q, double* Z, int masked, void* ws, size_t ws_bytes, void* stream);
/* Z[c] = colcnt[c] > 0 ? Z[c] / colcnt[c] * n_samples : 0     (missingvals.py:17-19) */
int cmtfpls_colscale_f64(double* Z, int64_t P, const double* colcnt, double n_samples, void* stream);

/* ---- K2 rank-1 extraction ----------------------------------------------------------------------
 * rank1: leading singular pair of the A x B matrix Z: what
 *   parafac(Z, 1, tol, init="svd", normalize_factors=True)[1]   (tpls.py:86-88, cmtf.py:100-102)
 * returns for a matrix Z.  wA = u1, wB = v1 (unit norm), sigma[0] = sigma_1 (nullable); sign: the
 * largest-|.| entry of wB is positive, wA follows (sigma > 0).  Method: repeated squaring of the Gram
 * matrix of the smaller side (at most n_squarings launches, the ones after convergence return at
 * once), then one exact pass y = M^T seed, x = M y with Z itself.  info (nullable, 2 doubles):
 * info[0] = 1 if the squaring was seen to converge within n_squarings (else the caller should call
 * again with a larger budget), info[1] = squarings actually computed (budget hint for the next call).
 * Limit: min(A, B) <= 4096 (round 2: 1024), CMTFPLS_EUNSUPPORTED beyond.
 * Round 4: for min(A, B) <= 256 and n_squarings <= 31 the whole chain of squarings is ONE launch (its (n/16)^2 workgroups stay
 * resident and pass the 16-row panels of G_s to each other through 8-byte agent-scope stores whose value is their own flag, no
 * grid barrier, no fence); cmtfpls_rank1_launches_f64 always takes the launch-per-squaring form (same bits: what the tests
 * compare the chain with).
 * normalize: v /= ||v||_2, the vector case `Z / norm(Z)` (tpls.py:84, cmtf.py:98) and
 * `q /= norm(q)` (tpls.py:101); nrm (nullable) receives the norm. */
size_t cmtfpls_rank1_workspace_bytes(int A, int B);
int cmtfpls_rank1_f64(const double* Z, int A, int B, double* wA, double* wB, double* sigma, double* info,
                      int n_squarings, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_rank1_launches_f64(const double* Z, int A, int B, double* wA, double* wB, double* sigma, double* info,
                               int n_squarings, void* ws, size_t ws_bytes, void* stream);
/* The one-launch chain needs all of its workgroups resident at once: true on a GPU the process has to itself.  If a workgroup
 * waits in vain (tens of milliseconds: several processes sharing the card) the extraction returns NaN loadings and info =
 * [0, -1]; the caller then switches the chain off for the process (every entry that extracts a rank-1 pair takes the launch
 * form from then on) and repeats the call.  on = 2 (tests only): the chain runs with one row of its workgroups missing, which
 * exercises exactly that path. */
void cmtfpls_rank1_chain_enable(int on);
int cmtfpls_rank1_chain_enabled(void);
/* rank1 followed by the score of the M rows of S with the loading just formed, tq[m] = S[m,:] . (wA (x) wB) -- the pair every
 * iteration of the cross-covariance loop issues (tpls.py:84-90, then Y^T t = S w) -- with the extraction's last kernel and the
 * score in ONE launch when S has M <= 64 rows of >= 8192 elements (B even); any other shape runs the two entries one after the
 * other.  Same results as cmtfpls_rank1_f64 + cmtfpls_score_f64, bit for bit. */
int cmtfpls_rank1_score_f64(const double* Z, int A, int B, double* wA, double* wB, double* info, int n_squarings,
                            const double* S, int M, double* tq, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_normalize_f64(double* v, int64_t n, double* nrm, void* stream);
/* rank1_tensor: the same parafac call when Z is a TENSOR of order n = 3 .. 7 (X of order 4 .. 8; orders 4 and 5 are
 * exercised by tests/test_cmtf.py:18-21, tests/test_tpls.py:132-155): leading-left-singular-vector
 * init of every unfolding, ALS sweeps, stop when |d rec_error| < tol from the 2nd sweep on (<= 100
 * sweeps), as tensorly 0.9.0 publishes it.  dims: HOST array of the n mode sizes (each <= 1024);
 * factors: device (n x ld) row-major, row m = factor of mode m (columns past dims[m] are not written).  info (nullable, 2
 * doubles): [1, sweeps run] -- or [0, -1] with NaN factors and no sweep when the one-launch chain of squarings of one of the n
 * inits gave up (see cmtfpls_rank1_chain_enable: switch the chain off and repeat the call); the inits report through n info
 * pairs in the workspace, read by the ALS kernel: no host synchronisation.
 * kron: out[c] = a[c / nb] * b[c % nb] (builds wB of the factored loading from the trailing factors). */
size_t cmtfpls_rank1_tensor_workspace_bytes(const int* dims, int n);
int cmtfpls_rank1_tensor_f64(const double* Z, const int* dims, int n, double tol, double* factors, int ld,
                             double* info, int n_squarings, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_kron_f64(const double* a, int na, const double* b, int nb, double* out, void* stream);
/* rank1_sparse: SPARSE loadings at the call site of rank1 (tpls.py:84-90, cmtf.py:98-102; the reference itself only has dense
 * ones).  soft(v, lam): theta = lam * max_j |v_j|, out_j = sign(v_j) * max(|v_j| - theta, 0), 0 <= lam < 1 -- at least one entry
 * survives, thresholded entries are exactly 0.0.  In: (wA, wB) = the dense pair of the A x B matrix Z as cmtfpls_rank1_f64 left
 * it; out: the sparse pair after sweeps of
 *   a = soft(Z wB, lamA); a /= |a|_2;   b = soft(Z^T a, lamB); b /= |b|_2;   d = max(|a - wA|_inf, |b - wB|_inf); (wA, wB) = (a, b)
 * stopped when d < tol_s (tol_s = 0: exactly max_sweeps sweeps) or after max_sweeps, the last iterate kept.  info (nullable, 2
 * doubles) = [converged ? 1 : 0, sweeps run].  A zero a or b gives NaN loadings, as normalising a zero vector does.
 * ONE launch of ONE workgroup runs every sweep (no wait on any other workgroup); cmtfpls_rank1_sparse_form(A, B), host only: 1 = Z
 * staged in LDS once (Z, the vectors and the partial sums within 150 KB; 128 x 128 is inside), 2 = Z read from L2 / global memory
 * on every half-sweep, 0 = outside the limits.  16-byte loads of Z when B is even and Z 16-byte aligned.  Every sum in an order
 * fixed by the thread index, no atomics: a second call on the same input returns the same bits.
 * Checked in this order, before any pointer is read: CMTFPLS_EUNSUPPORTED unless 2 <= A, B <= 4096 and A * B <= 65536;
 * CMTFPLS_EINVAL for a lambda outside [0, 1), max_sweeps < 1 or tol_s < 0.  The workspace size is 0 (everything lives in LDS); ws
 * may be NULL.
 * soft_normalize: v <- soft(v, lam) / |soft(v, lam)|_2 in place, the vector case `Z / norm(Z)` (tpls.py:84, cmtf.py:98) with
 * sparsity; nrm (nullable) receives the norm.  1 <= n <= 2^24 (CMTFPLS_EUNSUPPORTED beyond), lam as above. */
size_t cmtfpls_rank1_sparse_workspace_bytes(int A, int B);
int cmtfpls_rank1_sparse_form(int A, int B);
int cmtfpls_rank1_sparse_f64(const double* Z, int A, int B, double* wA, double* wB, double lamA, double lamB, double tol_s,
                             int max_sweeps, double* info, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_soft_normalize_f64(double* v, int64_t n, double lam, double* nrm, void* stream);

/* ---- cross-covariance contraction (not a reference call site: an exact re-association of the loop)
 * xcov: S (M x P, row-major f64) = Y^T X_(0), i.e. S[m, c] = sum_i Y[i*ldy + m] * X[i, c], on the
 * f64 matrix cores (v_mfma_f64_16x16x4_f64), one read of X.  Inside one component u = Y q, hence
 * np.einsum(X, u) = sum_m q_m S[m] (tpls.py:83) and Y.T @ t = S_(0) kron(wA, wB) (tpls.py:100): the
 * inner loop of tpls.py:79-107 can then run on S alone with mode0_contract_f64 / rank1 / score_f64
 * applied to S.  masked != 0: NaN entries of X contribute 0.  Any M (the reference has no limit, tpls.py:100-102): one pass
 * over X per 64 responses, all through the same workspace (sized for min(M, 64) responses).
 * quadform: out[0] = (q - q_old)^T G (q - q_old) = |Y q - Y q_old|^2 for G = Y^T Y (tpls.py:103). */
size_t cmtfpls_xcov_workspace_bytes(int64_t I, int64_t P, int M);
int cmtfpls_xcov_f32(const float* X, int64_t I, int64_t P, const double* Y, int ldy, int M, double* S,
                     int masked, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_xcov_f64(const double* X, int64_t I, int64_t P, const double* Y, int ldy, int M, double* S,
                     int masked, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_quadform_f64(const double* G, int M, const double* q, const double* q_old, double* out, void* stream);
/* 16-bit storage of X (suffixes _bf16: bfloat16, _f16: IEEE half; X = the raw bits).  A 16-bit X is only ever READ: the element is
 * converted to f64 on load (both conversions are exact; NaN and Inf stay what they are) and everything after that is the f64
 * arithmetic of the f32 / f64 entries -- same arguments, workspaces, limits, `masked` semantics and fixed-order partial sums.
 * Entries: xcov, xcov_stats, score_contract (the rows form only: B % 8 == 0, 4096 <= A * B <= 16384), mttkrp (every shape of
 * the f32 entry, tile form), the S builds of the fold entries (kfold_xcov, kfold_wide_xcov, kfold_weighted_xcov) and the read-only
 * diagnostics passes (recon_r2, resid_rows, contrib_rows, selectivity_cols).  No other entry has a 16-bit form: whatever writes X
 * or has none runs on a float32 copy. */
int cmtfpls_xcov_bf16(const uint16_t* X, int64_t I, int64_t P, const double* Y, int ldy, int M, double* S,
                      int masked, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_xcov_f16(const uint16_t* X, int64_t I, int64_t P, const double* Y, int ldy, int M, double* S,
                     int masked, void* ws, size_t ws_bytes, void* stream);
/* xcov_deflate (round 3): the deflation X -= t (x) w (tpls.py:109; NaN stays NaN, values rounded to the storage type) AND the
 * cross-covariance S = Y^T X0 of the DEFLATED block (X0: NaN -> 0) AND ssq[0] = |X0|^2, in one read + write of X.  For blocks with
 * missing values inside the cross-covariance loop: their S cannot be carried across a deflation algebraically, so a component
 * cost a read + write (deflation) and a read (rebuild of S); Y is the already deflated Y (with the masked score's row rescale
 * folded into further columns, as for cmtfpls_xcov_*).  S equals deflating first and calling cmtfpls_xcov_* (masked) bit for bit.
 * M <= 64, A * B % 4 == 0 (CMTFPLS_EUNSUPPORTED otherwise).  ws: cmtfpls_xcov_ssq_workspace_bytes(I, A * B, M). */
int cmtfpls_xcov_deflate_f32(float* X, int64_t I, int A, int B, const double* Y, int ldy, int M, const double* t, const double* wA,
                             const double* wB, double* S, double* ssq, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_xcov_deflate_f64(double* X, int64_t I, int A, int B, const double* Y, int ldy, int M, const double* t, const double* wA,
                             const double* wB, double* S, double* ssq, void* ws, size_t ws_bytes, void* stream);
/* xcov_ssq (round 3): S as cmtfpls_xcov_* (unmasked) AND ssq[0] = sum_{i,c} (X[i,c] - mean[c])^2 from the same read of an
 * UNCENTRED X without missing values: |X - X_mean|^2, the denominator of R2X (util.py:7-20, tpls.py:115-117), for the fit that
 * never centres, writes or copies X.  (The f64 value of every element is formed for the matrix cores anyway.) */
size_t cmtfpls_xcov_ssq_workspace_bytes(int64_t I, int64_t P, int M);
/* xcov_stats (round 4): S as cmtfpls_xcov_* (unmasked, M <= 64) AND the statistics pass of tpls.py:61-71 from the same read of an
 * uncentred X: stats[0..P) = the column sums, stats[P..2P) = the column sums of squares (a missing value shows as a NaN in its
 * column's sum: the caller then takes cmtfpls_colstats_* and the masked forms).  With them mean = sum / I and
 * |X - X_mean|^2 = sum_c (sumsq_c - sum_c^2 / I): a fit on the uncentred tensor reads X ONCE before its first component. */
size_t cmtfpls_xcov_stats_workspace_bytes(int64_t I, int64_t P, int M);
int cmtfpls_xcov_stats_f32(const float* X, int64_t I, int64_t P, const double* Y, int ldy, int M, double* S, double* stats,
                           void* ws, size_t ws_bytes, void* stream);
int cmtfpls_xcov_stats_f64(const double* X, int64_t I, int64_t P, const double* Y, int ldy, int M, double* S, double* stats,
                           void* ws, size_t ws_bytes, void* stream);
int cmtfpls_xcov_stats_bf16(const uint16_t* X, int64_t I, int64_t P, const double* Y, int ldy, int M, double* S, double* stats,
                            void* ws, size_t ws_bytes, void* stream);
int cmtfpls_xcov_stats_f16(const uint16_t* X, int64_t I, int64_t P, const double* Y, int ldy, int M, double* S, double* stats,
                           void* ws, size_t ws_bytes, void* stream);
int cmtfpls_xcov_ssq_f32(const float* X, int64_t I, int64_t P, const double* Y, int ldy, int M, double* S, const double* mean,
                         double* ssq, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_xcov_ssq_f64(const double* X, int64_t I, int64_t P, const double* Y, int ldy, int M, double* S, const double* mean,
                         double* ssq, void* ws, size_t ws_bytes, void* stream);
/* One inner iteration of the loop on S (tpls.py:80-103 re-associated) issued by a single host call:
 * Z = sum_m q_cur[m] S[m,:] (only if first != 0), rank1(Z) -> (wA, wB, info), q_new = S (wA (x) wB) normalised,
 * du2 = (q_new - q_cur)^T G (q_new - q_cur).  Same results as the separate entries (since round 3 the contraction of the M-row S is
 * one launch without partial rows, and the extraction's last kernel shares a launch with the score: cmtfpls_rank1_score_f64);
 * ws_rank1 as cmtfpls_rank1_workspace_bytes(A, B); ws_contract is no longer used (kept in the signature).  M <= 64. */
int cmtfpls_xcov_iterate_f64(const double* S, int M, int A, int B, const double* q_cur, double* Z, double* wA,
                             double* wB, double* info, int n_squarings, double* q_new, const double* G, double* du2,
                             int first, void* ws_contract, size_t ws_contract_bytes, void* ws_rank1,
                             size_t ws_rank1_bytes, void* stream);
/* The same for SEVERAL coupled blocks and for blocks with missing values (cmtf.py:91-128 re-associated), one host call:
 * per block  Z_b = sum_m q_cur[m] S_b[m,:]  (first != 0 only; masked blocks: Z_b[c] *= n_samples / colcnt[c], missingvals.py:17-19),
 * the loading -- rank1(Z_b) for an order-3 block (A x B), Z_b / |Z_b| for a matrix block (order 2: A = 1, wA = [1] is the caller's) --
 * and tq_b = S2_b (wA (x) wB)  (S2: the cross-covariance with the masked score's row rescale folded into Y; null = S);
 * then q_new = mean_b tq_b (cmtf.py:120; tq of block b is row b of the nb x M matrix `tq`), normalised, and
 * du2 = (q_new - q_cur)^T G (q_new - q_cur).  Blocks of order 2 or 3, M <= 64; ws_rank1: the largest
 * cmtfpls_rank1_workspace_bytes(A, B) of the order-3 blocks. */
typedef struct {
  const double* S;        /* M x A*B */
  const double* S2;       /* M x A*B or null */
  const double* colcnt;   /* A*B observation counts or null (no missing values) */
  double n_samples;       /* rows of X over all ranks (used with colcnt) */
  int order;              /* 2 (matrix block, A == 1) or 3 */
  int A, B;
  int n_squarings;        /* order 3 */
  double* Z;              /* A*B */
  double* wA;             /* A */
  double* wB;             /* B */
  double* info;           /* order 3: {converged, squarings used} */
} cmtfpls_xcov_block;
int cmtfpls_xcov_iterate_blocks_f64(const cmtfpls_xcov_block* blocks, int nb, int M, const double* q_cur, double* tq, double* q_new,
                                    const double* G, double* du2, int first, void* ws_rank1, size_t ws_rank1_bytes, void* stream);
/* S carried across one deflation instead of rebuilt (tpls.py:109 and :113 applied to S = Y^T X_(0)):
 * with X+ = X - t w^T and Y+ = Y - yhat q^T (yhat = T b, the inner-regression prediction),
 *   S+ = S - ya w^T - q v^T,   ya = Y^T t (M, taken before Y is deflated),  v = X+^T yhat (P, from
 * cmtfpls_deflate_contract_yq_* with Y = yhat as an I x 1 matrix and q = [1]),  w[c] = wA[c/B] wB[c%B]. */
int cmtfpls_s_downdate_f64(double* S, int M, int A, int B, const double* ya, const double* wA, const double* wB,
                           const double* q, const double* v, void* stream);
/* v[c] -= sum_{j<k} coef[j] WA[(c/B)*ld + j] WB[(c%B)*ld + j]  (k <= 64; WA: A x ld, WB: B x ld row-major): the xcov loop without
 * writing X.  With X_a = X_0 - sum_{j<a} t_j w_j^T (tpls.py:109 unrolled) the deflated tensor is never formed:
 *   final score   t_a = X_0 w_a - sum_{j<a} t_j (w_j^T w_a)            (cmtfpls_score_* on X_0, then cmtfpls_y_deflate_f64 on t),
 *   down-date     v = X_{a+1}^T yhat = X_0^T yhat - sum_{j<=a} w_j (t_j^T yhat)   (cmtfpls_mode0_contract_* on X_0, then this entry),
 *   R2X           |X_{a+1}|^2 = |X_a|^2 - 2 t^T t_b + t^T t  (t_b: the block's own score, = t for one block):
 * two reads of X per component instead of a read and a read + write, and X_0 stays as centred. */
int cmtfpls_kr_axpy_f64(double* v, int A, int B, const double* WA, const double* WB, int ld, int k, const double* coef, void* stream);
/* axpy_scalar: y[i] -= a[0] * (x ? x[i] : 1) for n doubles, a on the device.  The two rank-one corrections that let the
 * cross-covariance loop run on the caller's UNCENTRED X without ever writing or copying it (round 3):
 *   X_c w = X w - (mean^T w) 1  (scores),   X_c^T yhat = X^T yhat - (1^T yhat) mean  (the down-date of S). */
int cmtfpls_axpy_scalar_f64(double* y, int64_t n, const double* a, const double* x, void* stream);
/* score_contract (round 3): ONE read of X gives a score and the contraction with it,
 *   t[i] = sum_c X[i,c] w[c] - shift[0] - sub_own[i],   c[i] = alpha (t[i] + add_other[i]),   Z = X^T c
 * (w[c] = wA[c/B] wB[c%B]; shift, sub_own, add_other nullable = 0): multi_mode_dot, tpls.py:97-99, followed by
 * np.einsum("i...,i->...", X, c), tpls.py:83, with a score the pass just formed.  It removes the second read of X per component
 * from the never-writing cross-covariance loop above: yhat = T b is a combination of the scores, so X_0^T yhat = sum_j b_j r_j with
 * r_j = X_0^T t_j kept from the pass that formed t_j.  sub_own = T[:, :a] (w_j^T w_a)_j makes t the score of the implicitly
 * deflated X_a; for coupled blocks (cmtf.py:120) add_other = the sum of the other blocks' scores and alpha = 1 / blocks make c the
 * block-averaged score the deflation uses, for the block that is read last.
 * A row lives in the registers of one 1024-thread workgroup (A * B <= 16384) or, beyond that (round 4: the 256 x 256 rows of
 * BASELINE configs[4]), of up to 16 co-resident workgroups that each hold a column slab and exchange the row's partial dot products
 * through 8-byte agent-scope stores (value = flag, no fence): B % (16 / sizeof) == 0, 512 * (16 / sizeof) <= A * B <= 16 * 16384 (f32 with
 * 4096 % B == 0) / 16 * 8192 (f64, other f32 rows), no missing values; CMTFPLS_EUNSUPPORTED otherwise (use cmtfpls_score_* + cmtfpls_mode0_contract_*).
 * csum (nullable): csum[0] = sum_i c[i] (the uncentred form's correction X_c^T c = X^T c - (1^T c) mean).
 * ws: cmtfpls_score_contract_workspace_bytes(I, A * B). */
size_t cmtfpls_score_contract_workspace_bytes(int64_t I, int64_t P);
int cmtfpls_score_contract_f32(const float* X, int64_t I, int A, int B, const double* wA, const double* wB, const double* shift,
                               const double* sub_own, const double* add_other, double alpha, double* t, double* Z, double* csum,
                               void* ws, size_t ws_bytes, void* stream);
int cmtfpls_score_contract_f64(const double* X, int64_t I, int A, int B, const double* wA, const double* wB, const double* shift,
                               const double* sub_own, const double* add_other, double alpha, double* t, double* Z, double* csum,
                               void* ws, size_t ws_bytes, void* stream);
int cmtfpls_score_contract_bf16(const uint16_t* X, int64_t I, int A, int B, const double* wA, const double* wB, const double* shift,
                                const double* sub_own, const double* add_other, double alpha, double* t, double* Z, double* csum,
                                void* ws, size_t ws_bytes, void* stream);
int cmtfpls_score_contract_f16(const uint16_t* X, int64_t I, int A, int B, const double* wA, const double* wB, const double* shift,
                               const double* sub_own, const double* add_other, double alpha, double* t, double* Z, double* csum,
                               void* ws, size_t ws_bytes, void* stream);
/* Opt-in mixed-precision forms of xcov and mttkrp for f32-stored X: v_mfma_f32_16x16x4_f32 (half the
 * matrix cycles of the f64 form, HBM-bound instead of matrix-pipe-bound).  X is exact; the other
 * operand is rounded once to f32; f32 accumulation only inside chains of 64 rows (xcov) / 256 columns
 * (mttkrp), every chain added into f64.  Same arguments, workspaces and outputs as the f64 forms. */
int cmtfpls_xcov_f32_mixed(const float* X, int64_t I, int64_t P, const double* Y, int ldy, int M, double* S,
                           int masked, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_mttkrp_f32_mixed(const float* X, int64_t I, int A, int B, const double* WA, const double* WB, int R,
                             double* out, int ldo, void* stream);

/* mttkrp: M (I x R, leading dim ldo) = X_(0) (WA (.) WB), M[i, r] = sum_c X[i,c] WA[c / B, r] WB[c % B, r],
 * WA (A x R) and WB (B x R) row-major f64, R <= 32, on the f64 matrix cores; the Khatri-Rao operand is never
 * materialised (round 3: for A % 16 == 0, B % 64 == 0, R <= 16 the matrix cores contract over one trailing mode with the
 * plain loading of that mode as operand and the other mode's loading is folded into the accumulators; otherwise the
 * product WA[j,r] WB[k,r] is formed from LDS per tile).  One pass over X replaces the R project-and-deflate passes of
 * predict / transform (tpls.py:133-142, 156-165) when X has no NaN:
 * T = M (I + triu(W^T W, 1))^{-1} (the R x R part is done by the caller).
 * CMTFPLS_EUNSUPPORTED when R > 32 or (A + B) * 16 * ceil(R / 16) doubles exceed 152 KB of LDS. */
int cmtfpls_mttkrp_f32(const float* X, int64_t I, int A, int B, const double* WA, const double* WB, int R,
                       double* out, int ldo, void* stream);
int cmtfpls_mttkrp_f64(const double* X, int64_t I, int A, int B, const double* WA, const double* WB, int R,
                       double* out, int ldo, void* stream);
int cmtfpls_mttkrp_bf16(const uint16_t* X, int64_t I, int A, int B, const double* WA, const double* WB, int R,
                        double* out, int ldo, void* stream);
int cmtfpls_mttkrp_f16(const uint16_t* X, int64_t I, int A, int B, const double* WA, const double* WB, int R,
                       double* out, int ldo, void* stream);

/* ---- K3 score contraction: multi_mode_dot(X, [w...], range(1, X.ndim))  tpls.py:97-99 ---------
 * t[i] = sum_c X[i,c] * wA[c / B] * wB[c % B].
 * rowcnt != NULL selects the masked form miss_mmodedot (missingvals.py:23-38): NaN entries
 * contribute 0 and t[i] = dot / rowcnt[i] * P (0/0 = NaN for an empty row, as the reference). */
int cmtfpls_score_f32(const float* X, int64_t I, int A, int B, const double* wA, const double* wB,
                      const double* rowcnt, double* t, void* stream);
int cmtfpls_score_f64(const double* X, int64_t I, int A, int B, const double* wA, const double* wB,
                      const double* rowcnt, double* t, void* stream);
/* score_s: the same contraction for the M rows of a cross-covariance S = Y^T X_(0) inside the xcov loop, tq[m] = S[m, :] . w
 * (= Y^T t, tpls.py:100).  Few long rows (M <= 64, P >= 8192) take one 1024-thread workgroup per row.  Kept apart from
 * cmtfpls_score_*: that kernel sums in another order, and the score of a SAMPLE must not depend on how many samples are
 * passed with it -- M is fixed for a fit, a batch size is not. */
int cmtfpls_score_s_f64(const double* S, int M, int A, int B, const double* wA, const double* wB, double* tq, void* stream);

/* Deflation of one component fused with the first contraction of the next (tpls.py:109 followed by
 * tpls.py:80-83 of the next pass of the component loop): X is deflated in place exactly as
 * cmtfpls_deflate_* does, and in the same sweep Z[c] = sum_i X_new[i,c] * (Y[i,:] . q) and
 * ssq[0] = sum of squares of the observed entries of X_new (R2X numerator) are formed.  One read + one
 * write of X instead of read + write + read.  Vector shapes with B % (16/sizeof(T)) == 0 and M <= 64
 * only (CMTFPLS_EUNSUPPORTED otherwise: deflate, then mode0_contract). */
size_t cmtfpls_deflate_contract_workspace_bytes(int64_t I, int64_t P);
int cmtfpls_deflate_contract_yq_f32(float* X, int64_t I, int A, int B, const double* t, const double* wA,
                                    const double* wB, const double* Y, int ldy, int M, const double* q, double* Z,
                                    int masked, double* ssq, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_deflate_contract_yq_f64(double* X, int64_t I, int A, int B, const double* t, const double* wA,
                                    const double* wB, const double* Y, int ldy, int M, const double* q, double* Z,
                                    int masked, double* ssq, void* ws, size_t ws_bytes, void* stream);
/* score + the partial sums of Y^T t (tpls.py:100, `Y.T @ X_scores`) of every workgroup's rows:
 * qpart is (cmtfpls_sweep_partials() x M) row-major; cmtfpls_q_update_f64 adds the rows in index order.
 * M <= 64 (CMTFPLS_EUNSUPPORTED otherwise: use score + gram_tn). */
int cmtfpls_score_gram_f32(const float* X, int64_t I, int A, int B, const double* wA, const double* wB,
                           const double* rowcnt, double* t, const double* Y, int ldy, int M, double* qpart,
                           void* stream);
int cmtfpls_score_gram_f64(const double* X, int64_t I, int A, int B, const double* wA, const double* wB,
                           const double* rowcnt, double* t, const double* Y, int ldy, int M, double* qpart,
                           void* stream);
/* The Y-side update of one iteration in one launch (tpls.py:100-103), every step optional:
 *   qpart != NULL : q[m] = sum_b qpart[b*M + m]  (b < nblk, fixed order)
 *   normalize != 0: q /= ||q||_2                                            (tpls.py:101)
 *   G != NULL     : du2[0] = (q - q_prev)^T G (q - q_prev) = |Y q - Y q_prev|^2 for G = Y^T Y (tpls.py:103)
 * A sharded fit calls it twice around the all-reduce of q (first the sum, then the rest).  M <= 64. */
int cmtfpls_q_update_f64(const double* qpart, int nblk, int M, double* q, int normalize, const double* G,
                         const double* q_prev, double* du2, void* stream);

/* ---- K6 rank-1 deflation: X -= outer([t, w_J, w_K])  tpls.py:109; cmtf.py:130-131 ------------
 * X[i,c] -= t[i] * wA[c / B] * wB[c % B] in place, one read + one write of X.
 * ssq_part (nullable, cmtfpls_sweep_partials() doubles): per-block partial sums of the squared
 * deflated entries, NaNs skipped: ||X_{a+1}||^2 = the numerator of calcR2X (util.py:13) because
 * X_c - factors_to_tensor(X_factors) IS the deflated tensor at observed positions. */
int cmtfpls_deflate_f32(float* X, int64_t I, int A, int B, const double* t, const double* wA,
                        const double* wB, double* ssq_part, void* stream);
int cmtfpls_deflate_f64(double* X, int64_t I, int A, int B, const double* t, const double* wA,
                        const double* wB, double* ssq_part, void* stream);

/* ---- K3 + K6 fused (transform / predict inner step, tpls.py:133-142, 156-165) -----------------
 * per row: t[i] = score (masked form when rowcnt != NULL), then the row is deflated with it while
 * still in registers.  Returns CMTFPLS_EUNSUPPORTED when a row does not fit one workgroup's
 * registers (P > 65536 for f32, 32768 for f64): call score + deflate instead. */
int cmtfpls_score_deflate_f32(float* X, int64_t I, int A, int B, const double* wA, const double* wB,
                              const double* rowcnt, double* t, double* ssq_part, void* stream);
int cmtfpls_score_deflate_f64(double* X, int64_t I, int A, int B, const double* wA, const double* wB,
                              const double* rowcnt, double* t, double* ssq_part, void* stream);

/* ---- which form an X sweep takes (host arithmetic only: no GPU call, works without a device) ------
 * Every sweep entry above picks one of many kernel instances and grid policies from the shape, the storage
 * type and the alignment of X.  sweep_form writes the name of the form the entry `op` would take into out
 * (n bytes, NUL-terminated), from the same host function the entry itself launches from:
 *   op: "colstats", "mode0_contract", "mode0_contract_yq", "center", "score", "score_gram", "deflate",
 *       "score_deflate", "deflate_contract_yq";  elem_bytes: 4 (f32) or 8 (f64);  X is I x (A * B);
 *   masked: the entry's masked flag / rowcnt != NULL (center: rowcnt is wanted);  M: responses (yq, score_gram);
 *   aligned16: X is 16-byte aligned.
 * Names look like "vec U4 FULL ilv blocks256", "rows1024 nv16 KC FULL parked masked", "narrow nvl2 op2"; a
 * shape the entry declines with CMTFPLS_EUNSUPPORTED gives "unsupported: <reason>" (status CMTFPLS_OK: the
 * query succeeded).  CMTFPLS_EINVAL: unknown op, arguments the entry itself refuses as invalid, n too small.
 * sweep_form_list writes every name `op` can give for that element size, one per line. */
int cmtfpls_sweep_form(const char* op, int elem_bytes, int64_t I, int A, int B, int masked, int M,
                       int aligned16, char* out, size_t n);
int cmtfpls_sweep_form_list(const char* op, int elem_bytes, char* out, size_t n);

/* ---- K4 / K5 / K7 / K11 small f64 algebra on tall-skinny operands ----------------------------
 * gram_tn:     C (a x b, row-major) = A^T B over I rows; A is (I x a) with leading dim lda, B is
 *              (I x b) with ldb.  Y.T @ t (tpls.py:100), T^T T and T^T u (normal equations of the
 *              lstsq at tpls.py:110-112), Y^T Y.   Any a, b (tiled 64 x 64).
 * rowdot:      u[i] = sum_m Y[i*ldy + m] * q[m]  (u = Y @ q, tpls.py:102); when u_old != NULL also
 *              du2[0] = sum_i (u_old[i] - u[i])^2   (norm(oldU - u), tpls.py:103).
 * scores_mean: out[i] = (Ts[0][i] + Ts[1][i] + ...) / nb   (np.average(Ts, axis=0), cmtf.py:120).
 * y_deflate:   Y[i,m] -= (sum_r T[i*ldt + r] * b[r]) * q[m]  (tpls.py:113); ssq[0] = ||Y||_F^2 after.
 * sum:         out[0] = sum of n doubles in a fixed order (closes every *ssq_part* array). */
size_t cmtfpls_small_workspace_bytes(void);
int cmtfpls_gram_tn_f64(const double* A, int lda, int a, const double* B, int ldb, int b, int64_t I,
                        double* C, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_rowdot_f64(const double* Y, int ldy, int M, int64_t I, const double* q, double* u,
                       const double* u_old, double* du2, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_scores_mean_f64(const double* Ts, int nb, int64_t I, double* out, void* stream);
int cmtfpls_y_deflate_f64(double* Y, int ldy, int M, int64_t I, const double* T, int ldt, int R,
                          const double* b, const double* q, double* ssq, void* ws, size_t ws_bytes,
                          void* stream);
int cmtfpls_sum_f64(const double* in, int64_t n, double* out, void* stream);

/* project_rows: transform / predict of samples WITH missing values (tpls.py:128-142 with miss_mmodedot, missingvals.py:23-38) from
 * ONE read of the uncentred X, nothing written: a workgroup keeps one row in registers and runs the reference's whole sequence
 * on it -- x - mean (rounded to the storage type, as the centred copy would be), the observation count, and for a = 0..R-1 the
 * masked score t_a = (sum_obs x w_a) * P / n_obs, scores[i*ld + a] = t_a, x -= t_a w_a (rounded to the storage type) --
 * instead of a centring pass and R read + write passes (cmtfpls_score_deflate_*).  WA (A x R), WB (B x R) row-major, mean (P,
 * nullable = 0).  A lane holds up to 16 vectors of 16 bytes: rows of up to 4096 vectors run in 256-thread workgroups, rows of
 * up to 16384 vectors (256 x 256 f32, BASELINE configs[4]) in 1024-thread workgroups of 128 registers per lane.
 * CMTFPLS_EUNSUPPORTED for longer rows, a trailing extent B that does not divide the workgroup stride (256 or 1024 times
 * 16 / sizeof(T) elements), or loadings beyond 144 KB of LDS: the caller keeps the passes.
 * project_rows2: the same for TWO COUPLED blocks sharing the sample mode (ctPLS.transform / predict with missing values,
 * cmtf.py:143-177,180-210): one workgroup holds the sample's row of both blocks, the score of a step is the mean of the two
 * masked block scores (np.average, cmtf.py:155,206) and deflates both.  Always 256-thread workgroups: the longer block may take
 * at most 16 vectors per lane and the shorter at most 4 (an I x 512 matrix block: one); beside a longer block of more than 8
 * vectors the shorter may take only one (instances (2|4|8, 1|4) and (16, 1)); otherwise CMTFPLS_EUNSUPPORTED. */
int cmtfpls_project_rows_f32(const float* X, int64_t I, int A, int B, int R, const double* WA, const double* WB,
                             const double* mean, double* scores, int ld, void* stream);
int cmtfpls_project_rows_f64(const double* X, int64_t I, int A, int B, int R, const double* WA, const double* WB,
                             const double* mean, double* scores, int ld, void* stream);
int cmtfpls_project_rows2_f32(const float* X0, int A0, int B0, const double* WA0, const double* WB0, const double* mean0,
                              const float* X1, int A1, int B1, const double* WA1, const double* WB1, const double* mean1,
                              int64_t I, int R, double* scores, int ld, void* stream);
int cmtfpls_project_rows2_f64(const double* X0, int A0, int B0, const double* WA0, const double* WB0, const double* mean0,
                              const double* X1, int A1, int B1, const double* WA1, const double* WB1, const double* mean1,
                              int64_t I, int R, double* scores, int ld, void* stream);
/* project_rows_idx / project_rows2_idx (round 4): the same sequence for the n_rows samples listed in `rows` (device array of
 * sample indices into X and scores) only.  The samples of a batch are independent (tpls.py:128-142 works row by row), so a
 * sample WITHOUT a missing value keeps the score of the one-pass form (cmtfpls_mttkrp_* + cmtfpls_unit_upper_solve_rows_f64)
 * and only the samples with one take the masked sequence: a batch with a few incomplete samples no longer pays the
 * arithmetic-bound sequence for all of them.  Shape limits as above; n_rows = 0 is a no-op. */
int cmtfpls_project_rows_idx_f32(const float* X, const int64_t* rows, int64_t n_rows, int A, int B, int R, const double* WA,
                                 const double* WB, const double* mean, double* scores, int ld, void* stream);
int cmtfpls_project_rows_idx_f64(const double* X, const int64_t* rows, int64_t n_rows, int A, int B, int R, const double* WA,
                                 const double* WB, const double* mean, double* scores, int ld, void* stream);
int cmtfpls_project_rows2_idx_f32(const float* X0, int A0, int B0, const double* WA0, const double* WB0, const double* mean0,
                                  const float* X1, int A1, int B1, const double* WA1, const double* WB1, const double* mean1,
                                  const int64_t* rows, int64_t n_rows, int R, double* scores, int ld, void* stream);
int cmtfpls_project_rows2_idx_f64(const double* X0, int A0, int B0, const double* WA0, const double* WB0, const double* mean0,
                                  const double* X1, int A1, int B1, const double* WA1, const double* WB1, const double* mean1,
                                  const int64_t* rows, int64_t n_rows, int R, double* scores, int ld, void* stream);

/* ---- collectives of the sharded loop for callers that drive this C ABI directly -----------------------
 * In-place all-reduce(sum) of a device buffer over the caller's RCCL communicator (an ncclComm_t passed as void*), on
 * `stream`: Z (P doubles) and Y^T t (M doubles) per direct iteration, T^T [T | u] per component, S per component with
 * the cross-covariance form.  The library does not link RCCL: ncclAllReduce is resolved at first use from the RCCL
 * already loaded in the process (the one the communicator came from), else from librccl.so.1 on the loader path;
 * CMTFPLS_EUNSUPPORTED when there is none.  (The Python package issues the same collectives through its own process group.) */
int cmtfpls_allreduce_sum_f64(void* comm, double* buf, size_t count, void* stream);
int cmtfpls_allreduce_sum_f32(void* comm, float* buf, size_t count, void* stream);

/* ---- K7 / K8 / projection fix-up without a host round trip ------------------------------------------
 * normal_solve: b (k entries, stride incb) = argmin |T b - u| from the k x k normal equations G b = g with
 *   G = T^T T, g = T^T u (row-major f64, k <= 64): `np.linalg.lstsq(T, u, rcond=-1)[0]` of tpls.py:110-112 /
 *   cmtf.py:135-137 restricted to the k = a + 1 non-zero score columns.  Cholesky of the equilibrated matrix
 *   diag(G)^(-1/2) G diag(G)^(-1/2) (the score columns differ in scale by orders of magnitude; the raw normal
 *   equations would square that spread); a column that is zero or dependent to working precision gets b = 0.
 * unit_upper_solve_rows: rows of M (I x R, leading dim ld) are overwritten by the rows of T solving
 *   T (I + triu(U, 1)) = M - 1 shift^T: the R x R part of the one-pass transform / predict (see cmtfpls_mttkrp_*).
 *   shift (R doubles, nullable = 0): mean^T W, the centring `X - X_mean` of tpls.py:130,153 moved behind the MTTKRP,
 *   (X - 1 mean^T) W = X W - 1 (mean^T W)^T, so that X is read once, uncentred, and never written.  nan_flag (one
 *   int, nullable, zeroed by the caller): set to 1 when M holds a NaN, i.e. a row of X had a missing value.
 * kr_gram: G (R x R) = (first ? 1 : G) .* scale * L^T L for one loading matrix L (n x R row-major): the Gram
 *   matrix of a Khatri-Rao product is the Hadamard product of the mode Grams; call once per mode.
 * khatri_rao: out ((na * nb) x R) = column-wise Kronecker product of Am (na x R) and Bm (nb x R)
 *   (tensorly.tenalg.khatri_rao as used by util.py:19, first matrix varying slowest).
 * recon: Xhat[i, c] = sum_r T[i*ldt + r] * WA[(c / B)*R + r] * WB[(c % B)*R + r] + mean[c]  for I rows, written
 *   in the storage type: factors_to_tensor (util.py:18-20) + X_mean as X_reconstructed uses it (tpls.py:188-189,
 *   cmtf.py:233-237), the Khatri-Rao operand never materialised; mean nullable.  Any shape (16-byte vectors when
 *   B % (16/sizeof(T)) == 0 and `out` is aligned, single elements otherwise). */
int cmtfpls_normal_solve_f64(const double* G, const double* g, int k, double* b, int incb, void* stream);
/* normal_solve_ws: the same solve for any k <= 1024 (the reference's lstsq has no limit on n_components,
 * tpls.py:110-112): k <= 64 is cmtfpls_normal_solve_f64 (ws may be null); beyond, the equilibrated matrix lives in the
 * caller's workspace (cmtfpls_normal_solve_workspace_bytes(k); 0 for k <= 64) -- same algorithm, same pivot rule. */
size_t cmtfpls_normal_solve_workspace_bytes(int k);
int cmtfpls_normal_solve_ws_f64(const double* G, const double* g, int k, double* b, int incb, void* ws, size_t ws_bytes,
                                void* stream);
int cmtfpls_unit_upper_solve_rows_f64(double* M, int64_t I, int ld, int R, const double* U, const double* shift, int* nan_flag,
                                      void* stream);
int cmtfpls_kr_gram_f64(const double* L, int n, int R, double* G, int first, double scale, void* stream);
/* Row a of that Gram matrix only: g[j] = (first ? 1 : g[j]) * sum_i L[i][j] L[i][a] for j < a -- w_j^T w_a, what the never-writing
 * cross-covariance loop needs per component (the score correction T[:, :a] g). */
int cmtfpls_kr_gram_row_f64(const double* L, int n, int R, int a, double* g, int first, void* stream);
int cmtfpls_khatri_rao_f64(const double* Am, int na, const double* Bm, int nb, int R, double* out, void* stream);
/* predict_rows: out[i, m] = mean[m] + sum_a S[i*lds + a] * Bm[a*M + m]: `X_projection @ coef_ @ Q^T + Y_mean` (tpls.py:143,
 * cmtf.py:177) applied to the device-resident scores, Bm = coef_ Q^T (R x M, formed by the caller); mean nullable. */
int cmtfpls_predict_rows_f64(const double* S, int64_t I, int lds, int R, const double* Bm, int M, const double* mean,
                             double* out, int ldo, void* stream);
int cmtfpls_recon_f32(const double* T, int64_t I, int ldt, int R, const double* WA, const double* WB, int A, int B,
                      const double* mean, float* out, void* stream);
int cmtfpls_recon_f64(const double* T, int64_t I, int ldt, int R, const double* WA, const double* WB, int A, int B,
                      const double* mean, double* out, void* stream);
/* recon_r2: the two sums of calcR2X(X - mean, factors_to_tensor(X_factors)) (util.py:7-15 as called at tpls.py:115-117,
 * cmtf.py:132-134) in ONE read of the original X, the reconstruction never materialised:
 *   out[0] = sum over finite x of (xhat - x)^2,  out[1] = sum over finite x of x^2,  x = X[i,c] - mean[c] (mean
 * nullable), xhat as in recon;  R2X = 1 - out[0] / out[1].  (The fit itself gets R2X from the deflation sweep; this
 * is the literal formula for callers of calcR2X and for checking that identity at full size.)  Any shape; R <= 16. */
size_t cmtfpls_recon_r2_workspace_bytes(int64_t I, int64_t P);
int cmtfpls_recon_r2_f32(const float* X, const double* T, int64_t I, int ldt, int R, const double* WA, const double* WB,
                         int A, int B, const double* mean, double* out, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_recon_r2_f64(const double* X, const double* T, int64_t I, int ldt, int R, const double* WA, const double* WB,
                         int A, int B, const double* mean, double* out, void* ws, size_t ws_bytes, void* stream);
/* 16-bit X: as cmtfpls_recon_r2_f32 on the upcast values, bit for bit (X = the raw bits, only ever read; NaN and Inf are skipped as
 * in f32).  A thread's 4 columns are one 8-byte load when B % 4 == 0 and X is 8-byte aligned: f32's thread-to-column mapping, so
 * every sum runs in its order.  The same holds for the _bf16 / _f16 forms of resid_rows, contrib_rows and selectivity_cols below. */
int cmtfpls_recon_r2_bf16(const uint16_t* X, const double* T, int64_t I, int ldt, int R, const double* WA, const double* WB,
                          int A, int B, const double* mean, double* out, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_recon_r2_f16(const uint16_t* X, const double* T, int64_t I, int ldt, int R, const double* WA, const double* WB,
                         int A, int B, const double* mean, double* out, void* ws, size_t ws_bytes, void* stream);

/* resid_rows: the residual of recon_r2 kept per sample and per variable (validate.sample_diagnostics), in ONE read of the
 * uncentred X (I x A*B, storage type, any alignment), the reconstruction never materialised.  With x = X[i,c] - mean[c]
 * (mean nullable) and e = x - sum_r T[i*ldt + r] WA[(c / B)*R + r] WB[(c % B)*R + r], over the entries with x finite (the
 * calcR2X mask, util.py:7-15):
 *   rows[3*i + 0] = sum_c e^2 (the Q residual / SPE),  rows[3*i + 1] = sum_c x^2,  rows[3*i + 2] = number of such entries;
 *   cols[2*c + 0] = sum_i e^2,  cols[2*c + 1] = sum_i x^2  (cols nullable: the column sums are skipped).
 * A NaN score row gives a NaN rows[3*i + 0].  Deterministic: partials per (column tile, row) and per (row block, column),
 * closed by fixed-order reduces; no atomics.  R <= 16 (CMTFPLS_EUNSUPPORTED beyond); ws: cmtfpls_resid_rows_workspace_bytes. */
size_t cmtfpls_resid_rows_workspace_bytes(int64_t I, int64_t P);
int cmtfpls_resid_rows_f32(const float* X, const double* T, int64_t I, int ldt, int R, const double* WA, const double* WB,
                           int A, int B, const double* mean, double* rows, double* cols, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_resid_rows_f64(const double* X, const double* T, int64_t I, int ldt, int R, const double* WA, const double* WB,
                           int A, int B, const double* mean, double* rows, double* cols, void* ws, size_t ws_bytes, void* stream);
/* 16-bit X: as cmtfpls_resid_rows_f32 on the upcast values, bit for bit (see cmtfpls_recon_r2_bf16). */
int cmtfpls_resid_rows_bf16(const uint16_t* X, const double* T, int64_t I, int ldt, int R, const double* WA, const double* WB,
                            int A, int B, const double* mean, double* rows, double* cols, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_resid_rows_f16(const uint16_t* X, const double* T, int64_t I, int ldt, int R, const double* WA, const double* WB,
                           int A, int B, const double* mean, double* rows, double* cols, void* ws, size_t ws_bytes, void* stream);

/* contrib_rows: per-mode contributions of a sample to its Q residual (SPE) and its Hotelling T^2 (validate.sample_contributions), in
 * ONE read of the uncentred X (I x A*B, storage type, any alignment), nothing of X's size written.  Output row i (0 <= i < n) reads
 * row src = rows ? rows[i] : i of X (src outside [0, I): NaN outputs, nothing read) with scores T[i*ldt + r] and T^2 direction
 * H[i*ldh + r].  With x = X[src,c] - mean[c] (mean nullable), c = j*B + k, W = WA[j*R + r] WB[k*R + r], over the entries with x finite:
 *   e = x - sum_r T W,  d = x sum_r H W;
 *   speA[i*A + j] = sum_k e^2,  speB[i*B + k] = sum_j e^2,  t2A[i*A + j] = sum_k d,  t2B[i*B + k] = sum_j d.
 * speA and t2A may both be NULL when A == 1 (a matrix block: they would repeat the row totals).  A NaN row of T or H gives NaN outputs
 * for that row only.  Deterministic: a workgroup owns whole rows and closes both sums in a fixed order; no atomics, no workspace.
 * R <= 16 and 2 A (R + 1) doubles (plus 16 KB) within the 160 KB LDS: CMTFPLS_EUNSUPPORTED beyond, before any launch. */
int cmtfpls_contrib_rows_f32(const float* X, int64_t I, const double* T, int ldt, const double* H, int ldh, int R, const double* WA,
                             const double* WB, int A, int B, const double* mean, const int64_t* rows, int64_t n, double* speA, double* speB,
                             double* t2A, double* t2B, void* stream);
int cmtfpls_contrib_rows_f64(const double* X, int64_t I, const double* T, int ldt, const double* H, int ldh, int R, const double* WA,
                             const double* WB, int A, int B, const double* mean, const int64_t* rows, int64_t n, double* speA, double* speB,
                             double* t2A, double* t2B, void* stream);
/* 16-bit X: as cmtfpls_contrib_rows_f32 on the upcast values, bit for bit (see cmtfpls_recon_r2_bf16): the same lanes along k, rows per
 * workgroup, LDS size and limits (the vector path also needs mean 16-byte aligned, as in f32). */
int cmtfpls_contrib_rows_bf16(const uint16_t* X, int64_t I, const double* T, int ldt, const double* H, int ldh, int R, const double* WA,
                              const double* WB, int A, int B, const double* mean, const int64_t* rows, int64_t n, double* speA, double* speB,
                              double* t2A, double* t2B, void* stream);
int cmtfpls_contrib_rows_f16(const uint16_t* X, int64_t I, const double* T, int ldt, const double* H, int ldh, int R, const double* WA,
                             const double* WB, int A, int B, const double* mean, const int64_t* rows, int64_t n, double* speA, double* speB,
                             double* t2A, double* t2B, void* stream);

/* selectivity_cols: the target-projection sums behind the selectivity ratio of every variable (validate.selectivity_ratio), in ONE
 * read of the uncentred X (I x P, storage type, any alignment), nothing of X's size written or copied.  Tau (I x M, row stride ldtau
 * >= M) is the fitted response; with x = X[i,c] - mean[c] formed in registers (mean nullable: x = X) and o = isfinite(x) when
 * masked != 0, o = 1 otherwise:
 *   a[m*P + c] = sum_i o x Tau[i,m],   d[m*P + c] = sum_i o Tau[i,m]^2,   s[c] = sum_i o x^2,   n[c] = sum_i o.
 * d is written only when masked != 0 (it may be NULL otherwise: without a mask d[m, c] = sum_i Tau[i,m]^2 for every c, which the
 * caller forms once).  f64 matrix cores with the tiling of cmtfpls_xcov_*; the masked form runs a second accumulator set (A = Tau^2,
 * B = the 0 / 1 mask) and so takes 32 responses per pass over X where the complete form takes 64; more responses: more passes
 * inside the entry, s and n from the first.  Per-row-block partials closed in fixed order: no atomics, the same bits on every
 * call.  A non-finite row of Tau makes every output of its responses non-finite.  Argument errors (CMTFPLS_EINVAL) and a short
 * workspace (CMTFPLS_EWORKSPACE; ws: cmtfpls_selectivity_cols_workspace_bytes, enough for either form) are found before any launch. */
size_t cmtfpls_selectivity_cols_workspace_bytes(int64_t I, int64_t P, int M);
int cmtfpls_selectivity_cols_f32(const float* X, int64_t I, int64_t P, const double* Tau, int ldtau, int M, const double* mean,
                                 int masked, double* a, double* d, double* s, double* n, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_selectivity_cols_f64(const double* X, int64_t I, int64_t P, const double* Tau, int ldtau, int M, const double* mean,
                                 int masked, double* a, double* d, double* s, double* n, void* ws, size_t ws_bytes, void* stream);
/* 16-bit X: as cmtfpls_selectivity_cols_f32 on the upcast values, bit for bit (see cmtfpls_recon_r2_bf16).  The lane's 4 columns are one
 * 8-byte load when P % 4 == 0 and X is 8-byte aligned.  An f16 Inf (a value beyond 65504 when quantised) is masked as a NaN is. */
int cmtfpls_selectivity_cols_bf16(const uint16_t* X, int64_t I, int64_t P, const double* Tau, int ldtau, int M, const double* mean,
                                  int masked, double* a, double* d, double* s, double* n, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_selectivity_cols_f16(const uint16_t* X, int64_t I, int64_t P, const double* Tau, int ldtau, int M, const double* mean,
                                 int masked, double* a, double* d, double* s, double* n, void* ws, size_t ws_bytes, void* stream);

/* ---- imputation and entry-wise validation of the X model: validate.impute / validate.get_q2x_heldout (no reference counterpart;
 * the model they use is factors_to_tensor(X_factors) + X_mean, util.py:18-20 with tpls.py:188-189 / cmtf.py:233-237) ------------
 * THE HOLD-OUT RULE.  Element e of a block (C-order index) is held out iff
 *   unit_open(philox4x32_10(counter = (offset + e) / 4, stream, key = seed).v[(offset + e) % 4]) < fraction,
 * the generator of add_noise (Philox4x32-10, unit_open(x) = (x + 0.5) 2^-32).  stream = 2 + block index: streams 0 and 1 are the
 * noise and the NaN mask of add_noise.  offset = global index of the block's first element, so a row shard [a, b) of a block
 * with P columns, masked with offset = a P, is rows [a, b) of the whole block's mask.  No mask tensor exists anywhere: holdout_mask
 * and heldout_resid regenerate it from the counter.
 * Common to the three entries: X in its storage type (f32 / f64), everything else f64; 16-byte non-temporal vector accesses where
 * the buffers are 16-byte aligned (and, for heldout_resid / impute, B % (16 / sizeof(T)) == 0), single elements otherwise; sums
 * closed in a fixed order from per-workgroup partials in `ws` (no atomics: the same bits on every call); counts are doubles
 * (exact below 2^53).
 *
 * holdout_mask: out[e] = NaN where e is held out, else X[e] bit for bit (n elements; X is only read; out must not overlap X:
 *   CMTFPLS_EINVAL).
 *   counts[0] = entries newly hidden (held out and finite in X), counts[1] = finite entries left in out.
 *   One read, one write.  ws: cmtfpls_holdout_mask_workspace_bytes(n). */
size_t cmtfpls_holdout_mask_workspace_bytes(int64_t n);
int cmtfpls_holdout_mask_f32(const float* X, float* out, int64_t n, double fraction, uint64_t seed, uint32_t stream, uint64_t offset,
                             double* counts, void* ws, size_t ws_bytes, void* hipstream);
int cmtfpls_holdout_mask_f64(const double* X, double* out, int64_t n, double fraction, uint64_t seed, uint32_t stream, uint64_t offset,
                             double* counts, void* ws, size_t ws_bytes, void* hipstream);
/* heldout_resid: ONE read of the ORIGINAL X (I x A*B, uncentred).  With c = j*B + k and the prefix models
 *   xhat_r[i,c] = mean[c] + sum_{a<r} T[i*ldt + a] WA[j*R + a] WB[k*R + a]   (mean nullable; WA, WB as in recon; accumulated in
 *   component order, the running sum squared after each component),
 * over the entries that are held out (the rule above, e = i*A*B + c) AND finite:
 *   out[r-1] = sum (x - xhat_r)^2 for r = 1..R,   out[R] = sum (x - mean[c])^2,   out[R+1] = the number of such entries,
 * so that Q2X_r = 1 - out[r-1] / out[R].  R <= 16 (CMTFPLS_EUNSUPPORTED beyond); ws: cmtfpls_heldout_resid_workspace_bytes. */
size_t cmtfpls_heldout_resid_workspace_bytes(int64_t I, int64_t P, int R);
int cmtfpls_heldout_resid_f32(const float* X, int64_t I, int A, int B, const double* T, int ldt, int R, const double* WA, const double* WB,
                              const double* mean, double fraction, uint64_t seed, uint32_t stream, uint64_t offset, double* out,
                              void* ws, size_t ws_bytes, void* hipstream);
int cmtfpls_heldout_resid_f64(const double* X, int64_t I, int A, int B, const double* T, int ldt, int R, const double* WA, const double* WB,
                              const double* mean, double fraction, uint64_t seed, uint32_t stream, uint64_t offset, double* out,
                              void* ws, size_t ws_bytes, void* hipstream);
/* impute: out[i,c] = X[i,c] bit for bit where X[i,c] is finite, else xhat_R[i,c] (above) rounded once to the storage type.
 * out == X is allowed (on a private copy): then only the 16-byte vectors that held a non-finite entry are stored; out != X: every
 * vector is stored.  An out that overlaps X without being X: CMTFPLS_EINVAL.  count[0] = entries imputed.  R <= 16 (CMTFPLS_EUNSUPPORTED beyond); ws: cmtfpls_impute_workspace_bytes. */
size_t cmtfpls_impute_workspace_bytes(int64_t I, int64_t P);
int cmtfpls_impute_f32(const float* X, float* out, int64_t I, int A, int B, const double* T, int ldt, int R, const double* WA,
                       const double* WB, const double* mean, double* count, void* ws, size_t ws_bytes, void* hipstream);
int cmtfpls_impute_f64(const double* X, double* out, int64_t I, int A, int B, const double* T, int ldt, int R, const double* WA,
                       const double* WB, const double* mean, double* count, void* ws, size_t ws_bytes, void* hipstream);

/* ---- leave-one-out refits, all folds in one launch: validate.get_q2y  (cmtf_pls/validate.py:7-37) ------------
 * For every fold i in [fold0, fold0 + nfolds): a complete tPLS fit (tpls.py:73-113; R components, tol, max_iter, the
 * reference's loop and convergence test) on the I - 1 samples other than i, then predict (tpls.py:122-143) of sample
 * i into Ypred[i, :].  One workgroup per fold; X (I x A*B) and Y (I x M) are the ORIGINAL float64 data; colsum_x /
 * colsum_y are their column sums (fold means are down-dated from them).  n_iter (nullable, I x R ints): inner
 * iterations executed.  ws >= nfolds * cmtfpls_loo_fold_workspace_bytes(...).  X of order 2 (A = 1) or 3 without
 * missing values; CMTFPLS_EUNSUPPORTED when min(A, B) > 64, M > 64, R > 16 or the per-fold vectors exceed the LDS
 * (the caller then refits per fold with the regular entry points). */
size_t cmtfpls_loo_fold_workspace_bytes(int I, int A, int B, int M, int R);
int cmtfpls_loo_tpls_f64(const double* X, const double* Y, const double* colsum_x, const double* colsum_y, int I, int A,
                         int B, int M, int R, double tol, int max_iter, int fold0, int nfolds, double* Ypred,
                         int* n_iter, void* ws, size_t ws_bytes, void* stream);
/* loo_xcov (round 4): the same leave-one-out refits for trailing shapes BEYOND the LDS-resident form -- min(A, B) <= 256 (128 x 128,
 * 256 x 256), M <= 128 (second session of round 4: 64 before), R <= 64 -- one 1024-thread workgroup per fold.  The fold's means are down-dated from the column sums; inside a
 * component the NIPALS loop runs on the fold's cross-covariance S = Y_f^T X_f (M x P, formed once per component: tpls.py:83 becomes
 * S^T q, tpls.py:100 becomes S w, tpls.py:103 the quadratic form with Y_f^T Y_f), so an inner iteration reads 2 M P doubles
 * instead of the fold's 2 I P; the rank-1 extraction squares the n x n Gram matrix on the f64 matrix cores inside the workgroup.
 * Same arguments and results as cmtfpls_loo_tpls_f64 (which it equals to rounding where both apply);
 * ws >= nfolds * cmtfpls_loo_xcov_fold_workspace_bytes(...) (a centred copy of X per resident fold, deflated in place). */
size_t cmtfpls_loo_xcov_fold_workspace_bytes(int I, int A, int B, int M, int R);
int cmtfpls_loo_xcov_f64(const double* X, const double* Y, const double* colsum_x, const double* colsum_y, int I, int A,
                         int B, int M, int R, double tol, int max_iter, int fold0, int nfolds, double* Ypred,
                         int* n_iter, void* ws, size_t ws_bytes, void* stream);
/* loo_xcov_tensor: cmtfpls_loo_xcov_f64 for X of order 4 (I x A x B1 x B2), seen as I x A x B with B = B1 * B2: the same kernel, one
 * 1024-thread workgroup per fold, whose extraction is the reference's parafac(Z, 1, tol, init="svd", normalize_factors=True) on the
 * fold's A x B1 x B2 cross-covariance inside the workgroup (the rank-1 CP of cmtfpls_kfold_inner_tensor_f64) and whose loading of the
 * trailing modes is wK (x) wL (C order); score, deflation and held-out prediction are those of cmtfpls_loo_xcov_f64.  B2 = 1 (or
 * B1 = 1) is still a tensor: the CP runs, as on the regular engine.  Same arguments and results otherwise.  Checked on the host
 * before the launch: CMTFPLS_EINVAL for a bad pointer or size (any of A, B1, B2 <= 0); CMTFPLS_EUNSUPPORTED when the shorter side of
 * one of the three unfoldings of A x B1 x B2 exceeds 256, M > 128, R > 64, A * B1 * B2 > 2^24 or the workgroup's vectors exceed 150 KB
 * of LDS: (A + 2 B + 4 M + M^2 + n + B1 + B2 + max(A, B1, B2) + 1024 + 2 R^2 + R M + 3 R) doubles, n the largest of those shorter
 * sides (wA, wB, q, qn, tq, my, G_y, the Gram seed, then the CP's wK, wL, v, unscaled contraction and 1024 row-group partials, then
 * coef, Q, the normal equations); CMTFPLS_EWORKSPACE below nfolds * cmtfpls_loo_xcov_tensor_fold_workspace_bytes(...): per fold
 * (I P + I M + I R + M P + 6 P + 2 n^2 + 2 I + R (A + B)) doubles, P = A B (cmtfpls_loo_xcov_f64's with the CP's three length-P
 * scratch vectors).
 * cmtfpls_loo_xcov_tensor_lds_bytes (host only): the LDS of a workgroup as the launch sizes it, in doubles A + 2 B1 B2 + 4 M + M^2 + n +
 * B1 + B2 + max(A, B1, B2) + 1024 + 2 R^2 + R M + 3 R with the n above.  0 for a size <= 0 alone: a shape past a limit of the entry
 * (a short side, M, R, the cells, the 150 KB) still gets its byte count. */
size_t cmtfpls_loo_xcov_tensor_fold_workspace_bytes(int I, int A, int B1, int B2, int M, int R);
size_t cmtfpls_loo_xcov_tensor_lds_bytes(int A, int B1, int B2, int M, int R);
int cmtfpls_loo_xcov_tensor_f64(const double* X, const double* Y, const double* colsum_x, const double* colsum_y, int I, int A,
                                int B1, int B2, int M, int R, double tol, int max_iter, int fold0, int nfolds, double* Ypred,
                                int* n_iter, void* ws, size_t ws_bytes, void* stream);
/* loo_xcov_coupled: cmtfpls_loo_xcov_f64 for a COUPLED model (ctPLS, cmtf.py:85-177) on complete data: one 1024-thread workgroup per
 * held-out sample runs the whole fit of the other I - 1 samples on up to 8 blocks that share one score, and predicts its own row.
 * Every block's and Y's means are down-dated from the column sums; per component S_b = Y_f^T X_{b,f} (M x P_b) of every block and
 * G_y = Y_f^T Y_f are formed once and the inner loop runs on them from q = e_0, blocks in list order: Z_b = S_b^T q, w_b by
 * Z_b / |Z_b| (order 2) or the leading singular pair (order 3, Gram squarings on the f64 matrix cores),
 * Y^T t = (1 / nb) sum_b S_b (wA_b (x) wB_b), |u_old - u|^2 = dq^T G_y dq, no stop on the first pass; then t = mean_b X_{b,f} w_b,
 * every block deflated by its own t (x) w_b, coef from the normal equations of T, Y deflated.  The original blocks are only read.
 * Only rows fold0 .. fold0 + nfolds - 1 of Ypred (I x M) and n_iter (nullable, I x R) are written.
 * Checked on the host before the launch, in this order: CMTFPLS_EINVAL for a bad pointer or size (as cmtfpls_loo_xcov_f64; a block
 * without X or colsum, A or B <= 0, order < 2, or order 2 with A != 1); CMTFPLS_EUNSUPPORTED for nb > 8, a block of order > 3,
 * min(A_b, B_b) > 256, M > 128, R > 64, P_b = A_b B_b > 2^24, or more than 150 KB of LDS, which cmtfpls_loo_xcov_coupled_lds_bytes
 * returns: (sum A_b + sum B_b + 4 M + M^2 + nmax + kmax + 2 R^2 + R M + 3 R) doubles with nmax = max_b min(A_b, B_b) and
 * kmax = max_b max(A_b, B_b) (every block's wA, wB resident; the extraction scratch shared and sized for the largest block);
 * CMTFPLS_EWORKSPACE below nfolds * cmtfpls_loo_xcov_coupled_fold_workspace_bytes(...): per fold ((I + M) sumP + 3 Pmax + 2 nmax^2 +
 * I (M + R + 2) + R (sum A_b + sum B_b)) doubles, sumP = sum_b P_b, Pmax = max_b P_b.  With one block both formulas are
 * cmtfpls_loo_xcov_f64's.  The two size functions return 0 for a bad argument (nb outside 1..8 included). */
typedef struct {
  const double* X;        /* I x A*B row-major, the original block, no missing values */
  const double* colsum;   /* A*B: column sums over all I samples */
  int order;              /* 2 (a matrix: A = 1) or 3; 4 (B = B1 B2) for cmtfpls_loo_xcov_coupled_tensor_f64 alone */
  int A, B;
} cmtfpls_loo_coupled_block;
size_t cmtfpls_loo_xcov_coupled_fold_workspace_bytes(const cmtfpls_loo_coupled_block* blocks, int nb, int I, int M, int R);
size_t cmtfpls_loo_xcov_coupled_lds_bytes(const cmtfpls_loo_coupled_block* blocks, int nb, int I, int M, int R);
int cmtfpls_loo_xcov_coupled_f64(const cmtfpls_loo_coupled_block* blocks, int nb, const double* Y, const double* colsum_y, int I,
                                 int M, int R, double tol, int max_iter, int fold0, int nfolds, double* Ypred, int* n_iter,
                                 void* ws, size_t ws_bytes, void* stream);
/* loo_xcov_coupled_tensor: cmtfpls_loo_xcov_coupled_f64 with blocks of order 4 among blocks of order 2, 3 and 4 (cmtf.py:98-104 on an
 * order-3 Z_b: parafac(Z_b, 1, init="svd"), as cmtfpls_loo_xcov_tensor_f64).  `dims` is a HOST array of 2 nb ints, (B1_b, B2_b) for a
 * block of order 4 (blocks[b].order == 4, I x A_b x B1_b x B2_b seen as I x A_b x B_b with B_b = B1_b B2_b; B2_b = 1 is still a tensor)
 * and (0, 0) for a block of order 2 or 3 (cmtfpls_kfold_inner_coupled_tensor_f64's convention).  A 512-thread workgroup per fold; a
 * tensor block's extraction is the rank-1 CP of its A x B1 x B2 Z_b inside the workgroup, which leaves wB_b = wK_b (x) wL_b (C order);
 * everything after the extraction, and every block of order 2 or 3, is cmtfpls_loo_xcov_coupled_f64's arithmetic in its order.
 * Checked on the host before the launch, in this order: CMTFPLS_EINVAL for what cmtfpls_loo_xcov_coupled_f64 calls a bad argument or
 * block, dims == NULL, a negative dim, B1 B2 != B in a block of order 4, order 4 with B2 = 0 or another order with B2 > 0, order > 4,
 * or no block of order 4 at all (that is cmtfpls_loo_xcov_coupled_f64's call); CMTFPLS_EUNSUPPORTED for nb > 8, min(A_b, B_b) > 256 in
 * a block of order 2 or 3, an unfolding of a tensor block's A x B1 x B2 with its shorter side > 256, M > 128, R > 64,
 * P_b = A_b B_b > 2^24, or more than 150 KB of LDS, which cmtfpls_loo_xcov_coupled_tensor_lds_bytes returns:
 * (sum A_b + sum B_b + 4 M + M^2 + nmax + kmax + 2 R^2 + R M + 3 R + max B1 + max B2 + max B1 B2 + max dim + 512) doubles, nmax the
 * largest of min(A_b, B_b) over the blocks of order 2 or 3 and of the shorter side of each of the three unfoldings of every tensor
 * block, kmax = max max(A_b, B_b) over the blocks of order 2 or 3 alone (0 without one), the last five terms the CP's wK, wL, v, tmp
 * (the largest single dim A, B1 or B2) and the workgroup's partial sums, taken over the tensor blocks, which share them;
 * CMTFPLS_EWORKSPACE below nfolds * cmtfpls_loo_xcov_coupled_tensor_fold_workspace_bytes(...): per fold ((I + M) sumP + 3 Pmax +
 * 3 Ptmax + 2 nmax^2 + I (M + R + 2) + R (sum A_b + sum B_b)) doubles, Ptmax the largest P_b of a tensor block (the CP's U, yl, vr).
 * The two size functions return 0 for what the entry answers with CMTFPLS_EINVAL, for nb > 8 and for P_b > 2^24. */
size_t cmtfpls_loo_xcov_coupled_tensor_fold_workspace_bytes(const cmtfpls_loo_coupled_block* blocks, int nb, const int* dims, int I,
                                                            int M, int R);
size_t cmtfpls_loo_xcov_coupled_tensor_lds_bytes(const cmtfpls_loo_coupled_block* blocks, int nb, const int* dims, int I, int M, int R);
int cmtfpls_loo_xcov_coupled_tensor_f64(const cmtfpls_loo_coupled_block* blocks, int nb, const int* dims, const double* Y,
                                        const double* colsum_y, int I, int M, int R, double tol, int max_iter, int fold0, int nfolds,
                                        double* Ypred, int* n_iter, void* ws, size_t ws_bytes, void* stream);
/* ---- cross-validation refits of a tPLS whose X has missing values, all folds in one launch: validate.get_q2y / kfold_predictions
 * with EngineOptions.masked_folds (cmtf_pls/validate.py:7-37; tpls.py:61-63 X_hasMiss; missingvals.py:7-38) -------------------
 * For every fold f in [fold0, fold0 + nfolds): a complete tPLS fit (tpls.py:73-113) on the rows r with fold_of[r] != f, with the
 * reference's missing-value arithmetic when one of those rows has a missing entry (miss_tensordot: the column sum / c_p * n_f, 0
 * where c_p = 0; miss_mmodedot: the row sum / o_r * P; deflation of observed entries only), then predict (tpls.py:122-143) of
 * the held-out rows, centred by the fold's means and THEN masked (a column without a training observation has a NaN mean, so its
 * held-out entries count as missing), with the masked score for the whole batch when any held-out entry is missing.
 * Ypred[((r - 1) * I + i) * M + m] (R x I x M) = the prediction of held-out row i with the first r components (coef_ is upper
 * triangular).  One workgroup per fold.  X (I x A*B, NaN = missing) and Y (I x M, complete) are the ORIGINAL float64 data;
 * colsum_x / colcnt_x = cmtfpls_colstats_f64 of X (the fold's counts and means are down-dated from them), colsum_y the column sums
 * of Y; leave-one-out is fold_of = 0..I-1, K = I.  n_iter (nullable, K x R): inner iterations; status (K): 0 ok, 1 a training
 * row without an observed entry (the reference is NaN everywhere: refit or decline), 2 fewer than 2 training rows; info
 * (nullable, K x 2): [f, 0] = 1 when the training rows took the masked arithmetic, [f, 1] = 1 when the held-out batch did.
 * ws >= nfolds * cmtfpls_cv_masked_fold_workspace_bytes(...) (Xf | Yf | T per resident fold, deflated in place, and the fold's
 * column counts and means).  CMTFPLS_EUNSUPPORTED (checked before the workspace) when K > I, min(A, B) > 64, M > 64, R > 16 or
 * the per-fold vectors and per-row counts exceed 150 KB of LDS. */
size_t cmtfpls_cv_masked_fold_workspace_bytes(int I, int A, int B, int M, int R);
int cmtfpls_cv_masked_f64(const double* X, const double* Y, const int* fold_of, int K, const double* colsum_x,
                          const double* colcnt_x, const double* colsum_y, int I, int A, int B, int M, int R, double tol,
                          int max_iter, int fold0, int nfolds, double* Ypred, int* n_iter, int* status, int* info, void* ws,
                          size_t ws_bytes, void* stream);
/* ---- refits of a tPLS whose X has missing values on count-weighted rows, all models of a chunk in one launch: the permutation
 * test, repeated K-fold and the bootstrap (validate.py) with EngineOptions.masked_folds ------------------------------------------
 * Model m in [model0, model0 + nmodels) of nm: counts[m * I + r] >= 0 copies of X row r paired with Y row yrow[m * I + r]
 * (yrow nullable: identity) are its training data; counts 0 are held out.  A complete tPLS fit (tpls.py:73-113) on that literal
 * data, with the reference's missing-value arithmetic when some column has fewer weighted observations than n = sum_r counts
 * (every sum over rows weighted by the counts: means, miss_tensordot's c_p and n, q, the convergence norm, the normal equations of
 * the inner regression), then predict (tpls.py:122-143) of the held-out rows as one batch, as cmtfpls_cv_masked_f64 does.
 * Ypred[(((m * R) + r - 1) * I + i) * M + j] (nm x R x I x M, written at held-out rows only) = the prediction of held-out row i
 * with the first r components.  Factors (nullable, written by every model without a status): Wa (nm x R x A), Wb (nm x R x B),
 * coef (nm x R x R, coef_[row, component]), Q (nm x R x M).  n_iter (nullable, nm x R); status (nm): 0 ok, 1 a training row
 * without an observed entry, 2 n < 2, 3 a negative count or a yrow outside 0..I-1; info (nullable, nm x 2): whether the training
 * rows / the held-out batch took the masked arithmetic.  X (I x A*B, NaN = missing) and Y (I x M, complete) are the ORIGINAL
 * float64 data.  One workgroup per model.  ws >= nmodels * cmtfpls_cv_masked_model_workspace_bytes(...) (Xf | Yf | T per resident
 * model, deflated in place, and the model's column counts and means).  CMTFPLS_EUNSUPPORTED (checked before the workspace) when
 * min(A, B) > 64, M > 64, R > 16 or the per-model vectors and per-row counts exceed 150 KB of LDS. */
size_t cmtfpls_cv_masked_model_workspace_bytes(int I, int A, int B, int M, int R);
int cmtfpls_cv_masked_models_f64(const double* X, const double* Y, const int* counts, const int* yrow, int nm, int I, int A,
                                 int B, int M, int R, double tol, int max_iter, int model0, int nmodels, double* Ypred,
                                 double* Wa, double* Wb, double* coef, double* Q, int* n_iter, int* status, int* info,
                                 void* ws, size_t ws_bytes, void* stream);
/* ---- the same two entries for X of order 4 (I x A x B1 x B2, NaN = missing) with EngineOptions.masked_tensor_folds ---------------
 * cmtfpls_cv_masked_f64 / cmtfpls_cv_masked_models_f64 on the I x A x B view with B = B1 B2 (tpls.py:73-113 with miss_tensordot /
 * miss_mmodedot, missingvals.py:7-38, on that view): the fold's or model's Z (A x B1 x B2, already / c_p * n when it is masked)
 * goes through the rank-1 CP of the complete-data order-4 forms (tpls.py:86-88 on a tensor Z: parafac(Z, 1, init="svd",
 * normalize_factors=True), as cmtfpls_rank1_tensor_f64 states it), and wA with wB = wK (x) wL (C order) feed every other step
 * unchanged: means, masked score / o_r * P, deflation on the observed entries, inner regression, the held-out batch centred then
 * masked, status 1 / 2 / 3, info.  One 512-thread workgroup per fold or model.  Arguments as the order-3 entries with B1, B2 in
 * place of B; the models entry writes Wk (nm x R x B1) and Wl (nm x R x B2) (both nullable) in place of Wb.
 * ws >= n * cmtfpls_cv_masked_tensor_{fold,model}_workspace_bytes(...): per resident fold or model I P + I M + I R + 6 P doubles,
 * P = A B1 B2 (Xf | Yf | T | column counts | means | the CP's transpose, unfolding, long vector and right vector); 0 for I <= 1.
 * LDS of a workgroup, in doubles, with n the largest of min(A, B1 B2), min(B1, A B2), min(B2, A B1): 4 I + P + A + 2 B + 3 M +
 * 2 n^2 + n + 2 R^2 + R (A + B) + R M + 3 R + 512 + B1 + B2 + max(A, B1, B2) + 12.
 * CMTFPLS_EUNSUPPORTED (checked before the workspace and before any pointer is read) when that n > 64, M > 64, R > 16, the LDS
 * exceeds 150 KB, or, in the fold form, K > I.
 * cmtfpls_cv_masked_tensor_lds_bytes (host only) returns that LDS in bytes, as the launch of either entry sizes it; 0 for I <= 1 or
 * another size <= 0 alone: a shape past a limit of the entries still gets its byte count. */
size_t cmtfpls_cv_masked_tensor_lds_bytes(int I, int A, int B1, int B2, int M, int R);
/* reference: tpls.py:73-113, 122-143 (fit and predict of one fold), missingvals.py:7-38 */
size_t cmtfpls_cv_masked_tensor_fold_workspace_bytes(int I, int A, int B1, int B2, int M, int R);
/* reference: validate.py:24-33 (one refit per fold) over tpls.py:73-143 */
int cmtfpls_cv_masked_tensor_f64(const double* X, const double* Y, const int* fold_of, int K, const double* colsum_x,
                                 const double* colcnt_x, const double* colsum_y, int I, int A, int B1, int B2, int M, int R,
                                 double tol, int max_iter, int fold0, int nfolds, double* Ypred, int* n_iter, int* status,
                                 int* info, void* ws, size_t ws_bytes, void* stream);
/* reference: tpls.py:73-113, 122-143 (fit and predict of one model), missingvals.py:7-38 */
size_t cmtfpls_cv_masked_tensor_model_workspace_bytes(int I, int A, int B1, int B2, int M, int R);
/* reference: tpls.py:73-143 on literally repeated rows (X[idx], Y[idx]) */
int cmtfpls_cv_masked_tensor_models_f64(const double* X, const double* Y, const int* counts, const int* yrow, int nm, int I,
                                        int A, int B1, int B2, int M, int R, double tol, int max_iter, int model0, int nmodels,
                                        double* Ypred, double* Wa, double* Wk, double* Wl, double* coef, double* Q, int* n_iter,
                                        int* status, int* info, void* ws, size_t ws_bytes, void* stream);
/* ---- refits of a coupled model (ctPLS) whose blocks have missing values on count-weighted rows, all models of a chunk in one
 * launch: K-fold / leave-one-out Q2Y, the permutation test, repeated K-fold and the bootstrap (validate.py) with
 * EngineOptions.masked_folds_coupled (cmtf.py:69-139 fit with the per-block Xs_hasMiss / Xs_miss, cmtf.py:141-175 predict;
 * missingvals.py:7-38) ------------------------------------------------------------------------------------------------------------
 * The count-weighted model of cmtfpls_cv_masked_models_f64 for nb blocks that share one score.  Model m in [model0, model0 +
 * nmodels) of nm: counts[m * I + r] >= 0 copies of row r of EVERY block paired with Y row yrow[m * I + r] (yrow nullable:
 * identity); counts 0 are held out.  A complete ctPLS fit on that literal data, every sum over rows weighted by the counts, the
 * missing-value arithmetic per block: block b is masked when one of its columns has fewer weighted observations than n = sum_r
 * counts (Xs_hasMiss[b], cmtf.py:77); then miss_tensordot (cmtf.py:95) and miss_mmodedot (cmtf.py:111-117) for that block, the
 * plain sums (cmtf.py:93, 106-110) for a complete one; the blocks' scores averaged in block order (cmtf.py:119); every block
 * deflated by the shared score on its observed entries (cmtf.py:130-131); the inner regression on the weighted rows
 * (cmtf.py:136-138).  Then predict (cmtf.py:141-175) of the held-out rows as one batch: each block centred by the model's means and
 * THEN masked, block b of the batch masked when any of its entries is missing, the blocks' scores averaged, every block deflated by
 * the average; a held-out row with nothing observed in some block predicts NaN.
 * Ypred[(((m * R) + r - 1) * I + i) * M + j] (nm x R x I x M, written at held-out rows only) = the prediction of held-out row i
 * with the first r components.  Factors (nullable, written by every model without a status): Wa (nm x R sumA; model m's block b is
 * the R x A_b matrix at m * R * sumA + R * (A_0 + .. + A_(b-1))), Wb (nm x R sumB, likewise), coef (nm x R x R, coef_[row,
 * component]), Q (nm x R x M).  n_iter (nullable, nm x R); status (nm): 0 ok, 1 a training row without an observed entry in some
 * block, 2 n < 2, 3 a negative count or a yrow outside 0..I-1 (a model with a status writes nothing else); info (nullable, nm x 2):
 * bit b of [m, 0] = block b's training rows took the masked arithmetic, bit b of [m, 1] = block b's held-out batch did.
 * Every block's X (I x A*B, NaN = missing) and Y (I x M, complete) are the ORIGINAL float64 data.  One 256-thread workgroup per
 * model.  ws >= nmodels * cmtfpls_cv_masked_coupled_workspace_bytes(...): per resident model sum_b (I P_b + 2 P_b) + I M + I R
 * doubles (per block the working copy, deflated in place, and the model's column counts and means; then Yf | T).
 * cmtfpls_cv_masked_coupled_lds_bytes: the LDS of a workgroup, in doubles 3 I + 3 M + 2 R^2 + R M + 3 R + 256 + Pmax + 2 nmax^2 +
 * nmax + kmax + sum_b [(R + 1)(A_b + B_b) + I] with Pmax = max A_b B_b, nmax = max min(A_b, B_b), kmax = max max(A_b, B_b) (the
 * per-block scratch is shared by the blocks); 0 for a bad argument.
 * CMTFPLS_EUNSUPPORTED (checked before the workspace and before any pointer is read) when nb > 8, a block's order is not 2 or 3,
 * a block's min(A, B) > 64, M > 64, R > 16 or the LDS exceeds 150 KB. */
typedef struct {
  const double* X;        /* I x A*B row-major, the original block, NaN = missing */
  int order;              /* 2 (a matrix: A = 1) or 3; 4 (B = B1 B2) for cmtfpls_cv_masked_coupled_tensor_f64 alone */
  int A, B;
} cmtfpls_cv_coupled_block;
size_t cmtfpls_cv_masked_coupled_workspace_bytes(const cmtfpls_cv_coupled_block* blocks, int nb, int I, int M, int R);
size_t cmtfpls_cv_masked_coupled_lds_bytes(const cmtfpls_cv_coupled_block* blocks, int nb, int I, int M, int R);
int cmtfpls_cv_masked_coupled_f64(const cmtfpls_cv_coupled_block* blocks, int nb, const double* Y, const int* counts,
                                  const int* yrow, int nm, int I, int M, int R, double tol, int max_iter, int model0, int nmodels,
                                  double* Ypred, double* Wa, double* Wb, double* coef, double* Q, int* n_iter, int* status,
                                  int* info, void* ws, size_t ws_bytes, void* stream);
/* cmtfpls_cv_masked_coupled_f64 for a coupled model with blocks of order 4 next to blocks of order 2 and 3.  A block I x A x B1 x B2
 * is given as I x A*B with order 4 and B = B1 B2; dims is a HOST array of 2 nb ints, (B1, B2) for a block of order 4 and (0, 0) for
 * another (B2 = 1 is still a tensor).  Every step runs on the I x A x B view unchanged; only the loading of a tensor block differs:
 * the rank-1 CP of its contraction Z (A x B1 x B2, already / c_p * n when the block is masked) inside the workgroup
 * (parafac(Z, 1, tol, init="svd", normalize_factors=True), as cmtfpls_rank1_tensor_f64 states it), wB = wK (x) wL in C order.  One
 * 512-thread workgroup per model.  The arguments, outputs, status and info are cmtfpls_cv_masked_coupled_f64's (Wb of a tensor
 * block receives wK (x) wL), with Wk (nullable, nm x R sumB1; model m's tensor block b is the R x B1_b matrix at m * R * sumB1 +
 * R * (the B1 of the tensor blocks before b)) and Wl (nullable, nm x R sumB2, likewise), the sums over the tensor blocks only.
 * ws >= nmodels * cmtfpls_cv_masked_coupled_tensor_workspace_bytes(...): cmtfpls_cv_masked_coupled_workspace_bytes plus 4 Ptmax
 * doubles (the CP's Zt | U | yl | vr, Ptmax = max A_b B_b over the tensor blocks).
 * cmtfpls_cv_masked_coupled_tensor_lds_bytes: in doubles 3 I + 3 M + 2 R^2 + R M + 3 R + 512 + Pmax + 2 nmax^2 + nmax + kmax +
 * max B1 + max B2 + max B1 B2 + max(A, B1, B2) + 12 + sum_b [(R + 1)(A_b + B_b) + I], nmax over min(A_b, B_b) of the matrix blocks
 * and the shorter side of every unfolding of every tensor block, kmax over max(A_b, B_b) of the matrix blocks alone, the four maxima
 * over the tensor blocks; 0 for a bad argument or description.
 * CMTFPLS_EINVAL (before any pointer is read) for what cmtfpls_cv_masked_coupled_f64 calls a bad argument or block, dims == NULL, a
 * negative dim, B1 * B2 != B, order 4 with B2 = 0, another order with B2 > 0, order > 4, or no block of order 4 (that is
 * cmtfpls_cv_masked_coupled_f64's call).  CMTFPLS_EUNSUPPORTED when nb > 8, a matrix block's min(A, B) > 64, a tensor block has an
 * unfolding whose shorter side is > 64, M > 64, R > 16 or the LDS exceeds 150 KB. */
size_t cmtfpls_cv_masked_coupled_tensor_workspace_bytes(const cmtfpls_cv_coupled_block* blocks, int nb, const int* dims, int I, int M,
                                                        int R);
size_t cmtfpls_cv_masked_coupled_tensor_lds_bytes(const cmtfpls_cv_coupled_block* blocks, int nb, const int* dims, int I, int M, int R);
int cmtfpls_cv_masked_coupled_tensor_f64(const cmtfpls_cv_coupled_block* blocks, int nb, const int* dims, const double* Y,
                                         const int* counts, const int* yrow, int nm, int I, int M, int R, double tol, int max_iter,
                                         int model0, int nmodels, double* Ypred, double* Wa, double* Wb, double* Wk, double* Wl,
                                         double* coef, double* Q, int* n_iter, int* status, int* info, void* ws, size_t ws_bytes,
                                         void* stream);
/* ---- K-fold cross-validation with every fold served by the same reads of X (validate.kfold_predictions) ------------------------
 * The folds of a K-fold split share X_0 (the caller's uncentred tensor, never written); a fold differs only in its training rows,
 * their means and its loadings.  Per component: kfold_inner (the inner loop of every fold on its training cross-covariance, a
 * workgroup per fold), one MTTKRP of X_0 with the K folds' loadings (cmtfpls_mttkrp_*: every row's score under every fold),
 * kfold_epilogue stage 1 (scores, inner regression, Y side), one contraction X_0^T [t_k * train_k] (cmtfpls_xcov_*, all but the
 * last component) and kfold_epilogue stage 2 (the down-date of each fold's S).  Before the first component kfold_xcov builds the
 * training cross-covariances from ONE read and kfold_epilogue stage 0 the Grams of the folds' training Y.  2R reads of X for all
 * folds.  Limits: X of order 2 (A = 1) or 3 without missing values, 2 <= K <= 32, M <= 64, R <= 64, min(A, B) <= 256
 * (CMTFPLS_EUNSUPPORTED otherwise: refit per fold).  All device buffers below are float64, row-major, owned by the caller. */
typedef struct {
  int I, A, B, M, K, R;
  const int* fold_of;     /* I: fold id of each row */
  double* S;              /* K x M x A*B: each fold's training cross-covariance (centred; down-dated per component) */
  double* mean;           /* K x A*B: each fold's training column means */
  double* Yk;             /* K x I x M: each fold's training Y, centred by its mean and deflated; held-out rows 0 */
  double* Gy;             /* K x NT x M x M: per row tile the partial Yk^T Yk of the current component (NT = cmtfpls_kfold_row_tiles(I)) */
  double* WA;             /* A x K: the current component's loadings, column k = fold k (the MTTKRP operands) */
  double* WB;             /* B x K */
  double* Q;              /* K x R x M: q of every component */
  double* Wa;             /* K x R x A: loadings of every component */
  double* Wb;             /* K x R x B */
  double* T;              /* K x I x R: the score of every row under each fold's model */
  double* Gt;             /* K x R x R: Gram of the training scores */
  double* coef;           /* K x R x R: coef_ of each fold's model (upper triangular) */
  double* Rm;             /* K x R x A*B: X_c^T t_j of each fold's training rows */
  double* tm;             /* I x K: the current component's scores, 0 on each fold's held-out rows (contraction operand) */
  double* Tout;           /* I x R: each row's scores under the model of its own fold (the held-out projection) */
  double* vec;            /* K x (3 R + M + 2) scratch */
  int* n_iter;            /* K x R: inner iterations executed */
  int* status;            /* K: zeroed by the caller; nonzero = a non-finite loading or coefficient */
  double* part;           /* K x NT x cmtfpls_kfold_part_stride() scratch: the row tiles' partial sums */
} cmtfpls_kfold_state;
/* Row tiles of the epilogue's grid (partial sums added in tile order) and the stride of a tile's partials in `part`. */
int cmtfpls_kfold_row_tiles(int64_t I);
int cmtfpls_kfold_part_stride(void);
/* kfold_xcov: S[k] = X_c[train_k]^T (Y[train_k] - nu_k) for every fold from ONE read of X: the fold-grouped partials
 * X[rows_f]^T Y[rows_f] and column sums (rows in the order `order`, fold f = rows order[fold_off[f] .. fold_off[f+1])), then the
 * all-minus-own identity and a rank-one centring correction.  Y (I x M): the responses minus any constant shift c; ydev (K x M):
 * nu_k - c.  mean (K x A*B): the training means; stats (2 A*B): column sums and sums of squares of all rows.
 * ws >= cmtfpls_kfold_xcov_workspace_bytes(I, A * B, M, K). */
size_t cmtfpls_kfold_xcov_workspace_bytes(int64_t I, int64_t P, int M, int K);
int cmtfpls_kfold_xcov_f32(const float* X, int64_t I, int A, int B, const double* Y, int M, const int* order, const int* fold_off, int K,
                           const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_kfold_xcov_f64(const double* X, int64_t I, int A, int B, const double* Y, int M, const int* order, const int* fold_off, int K,
                           const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream);
/* 16-bit X (the raw bits, only ever read): every argument, workspace size, limit and status is that of _f32, and S, mean and stats
 * are the bits _f32 returns on the upcast values (each element is converted to f64 on load, exactly; the sums run in _f32's order).
 * NaN and Inf reach stats.  The same holds for the _bf16 / _f16 forms of kfold_wide_xcov and kfold_weighted_xcov below. */
int cmtfpls_kfold_xcov_bf16(const uint16_t* X, int64_t I, int A, int B, const double* Y, int M, const int* order, const int* fold_off, int K,
                            const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_kfold_xcov_f16(const uint16_t* X, int64_t I, int A, int B, const double* Y, int M, const int* order, const int* fold_off, int K,
                           const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream);
/* kfold_inner: component a's inner loop (tpls.py:78-107 on S, as cmtfpls_loo_xcov_f64) for every fold, a 1024-thread workgroup per
 * fold: writes WA / WB (columns k), Q[k, a], n_iter[k, a].  ws >= cmtfpls_kfold_inner_workspace_bytes(A, B, K). */
size_t cmtfpls_kfold_inner_workspace_bytes(int A, int B, int K);
int cmtfpls_kfold_inner_f64(const cmtfpls_kfold_state* st, int a, double tol, int max_iter, void* ws, size_t ws_bytes, void* stream);
/* kfold_inner_tensor: kfold_inner for X of order 4 (I x A x B1 x B2) seen as I x A x B with st->B == B1 * B2 (CMTFPLS_EINVAL
 * otherwise) and the Kronecker loading wB = wK (x) wL (C order); every other kfold entry takes that state unchanged.  The rank-1
 * extraction of the A x B1 x B2 cross-covariance is the rank-1 CP of cmtfpls_rank1_tensor_f64, run inside each fold's workgroup.
 * model_fold == NULL, groups == 1: the plain layout (also the split-major and weighted models); otherwise the grouped layout of
 * cmtfpls_kfold_inner_grouped_f64.  Wk (K x R x B1) and Wl (K x R x B2), nullable, receive the mode loadings of component a; all
 * else it writes is what cmtfpls_kfold_inner_f64 writes.  Limits, checked before the launch (CMTFPLS_EUNSUPPORTED): those of
 * kfold_inner, the shorter side of each of the three unfoldings of A x B1 x B2 <= 256, and the fold's vectors
 * (A + 2 B1 B2 + B1 + B2 + max dim + 3 M + M^2 + 1280 doubles at most) within 150 KB of LDS.
 * ws >= cmtfpls_kfold_inner_tensor_workspace_bytes(A, B1, B2, K).
 * cmtfpls_kfold_inner_tensor_lds_bytes (host only): the LDS of a workgroup as the launch sizes it, in doubles A + 2 B1 B2 + 3 M + M^2 +
 * n + B1 + B2 + max(A, B1, B2) + 1024 with n the largest of min(A, B1 B2), min(B1, A B2), min(B2, A B1) (wA, wB, q, qn, tq, G_y, the
 * Gram seed, then the CP's wK, wL, v, unscaled contraction and 1024 row-group partials).  0 for a size <= 0 alone: a shape past a
 * limit of the entry still gets its byte count. */
size_t cmtfpls_kfold_inner_tensor_workspace_bytes(int A, int B1, int B2, int K);
size_t cmtfpls_kfold_inner_tensor_lds_bytes(int A, int B1, int B2, int M);
int cmtfpls_kfold_inner_tensor_f64(const cmtfpls_kfold_state* st, const int* model_fold, int groups, int B1, int B2, int a, double tol,
                                   int max_iter, double* Wk, double* Wl, void* ws, size_t ws_bytes, void* stream);
/* kfold_epilogue: stage 0 = the partial Gy of every fold (before component 0; `in` unused); stage 1 = component a's epilogue from
 * `in` = the MTTKRP X_0 WA (.) WB (I x K): a grid of row tiles x folds for the row work, a small solve per fold; stage 2 = the down-date of S from `in` = X_0^T tm (K x A*B), not after the last component. */
int cmtfpls_kfold_epilogue_f64(const cmtfpls_kfold_state* st, int stage, int a, const double* in, void* stream);
/* K-fold cross-validation of a coupled model (ctPLS: nb blocks sharing the sample mode and one score t, the average of the
 * blocks' scores).  `blocks` holds nb <= 8 state views, one per block: S, mean, WA, WB, Wa, Wb, Rm, A and B are that block's
 * (A = 1 for a matrix block); every other field is the same buffer in all views (CMTFPLS_EINVAL otherwise).  Per component a:
 * kfold_inner_coupled; per block the MTTKRP X_b,0 WA_b (.) WB_b into row b of an nb x I x K stack; kfold_combine_scores of the
 * stack; kfold_epilogue stage 1 on blocks[0] with the combined scores; and, all but the last component, per block the contraction
 * X_b,0^T tm and kfold_epilogue stage 2 on blocks[b].  Before component 0: kfold_xcov per block (ydev shared), kfold_epilogue
 * stage 0 on blocks[0].  2R reads of each block for all folds.  Limits: every block within the limits of kfold_inner and
 * the blocks' vectors within 150 KB of LDS (CMTFPLS_EUNSUPPORTED otherwise). */
/* kfold_inner_coupled: component a's inner loop for every fold over all blocks, a 1024-thread workgroup per fold going through the
 * blocks in turn (Z_b = S_b^T q, rank-1 of Z_b -> w_b, q ∝ sum_b S_b w_b / nb, convergence on dq^T G_y dq): writes every block's
 * WA / WB (columns k) and Wa / Wb [k, a], the shared Q[k, a], n_iter[k, a], and in vec the block-averaged mu^T w and g.
 * ws >= cmtfpls_kfold_inner_coupled_workspace_bytes(blocks, nb) (reads A, B and K of the views). */
size_t cmtfpls_kfold_inner_coupled_workspace_bytes(const cmtfpls_kfold_state* blocks, int nb);
int cmtfpls_kfold_inner_coupled_f64(const cmtfpls_kfold_state* blocks, int nb, int a, double tol, int max_iter, void* ws, size_t ws_bytes,
                                    void* stream);
/* kfold_inner_coupled_tensor: kfold_inner_coupled for a coupled model with blocks of order 4.  `dims` is a HOST array of 2 nb ints,
 * (B1_b, B2_b) per block: (0, 0) for a matrix block (order 2 or 3, extracted as in kfold_inner_coupled); otherwise block b is
 * I x A_b x B1_b x B2_b seen as I x A_b x B_b with blocks[b].B == B1_b * B2_b (CMTFPLS_EINVAL otherwise), its extraction is the
 * rank-1 CP of cmtfpls_kfold_inner_tensor_f64 inside the fold's workgroup and its WB / Wb hold wK (x) wL (C order); B2_b = 1 is a
 * tensor (the CP runs).  Every other kfold entry takes the views unchanged.  model_fold == NULL, groups == 1: the plain layout (also
 * the split-major and weighted models); otherwise the grouped layout of cmtfpls_kfold_inner_coupled_grouped_f64 (every view's mean
 * per fold).  Wk / Wl, nullable, receive the mode loadings of component a: the tensor blocks' slices lie one after another in block
 * order, that of tensor block b being K x R x B1_b doubles in Wk and K x R x B2_b doubles in Wl (model k, component a at
 * [(k R + a) B1_b + j] of the slice; a matrix block has no slice); all else it writes is what cmtfpls_kfold_inner_coupled_f64
 * writes.  With one block of order 4 the result is bitwise that of cmtfpls_kfold_inner_tensor_f64.  Checked on the host before the
 * launch: CMTFPLS_EINVAL for nb, dims, model_fold / groups (as the grouped entry) and the view checks; CMTFPLS_EUNSUPPORTED for the
 * limits of kfold_inner_coupled, a tensor block with the shorter side of one of its three unfoldings > 256, and the blocks' vectors
 * (max A + max B + 3 M + M^2 + n + k + max B1 + max B2 + max B1 B2 + max dim + 1024 doubles: n the largest short side over every
 * matrix block and every unfolding, k the largest long side of a matrix block, the other maxima over the tensor blocks) beyond
 * 150 KB of LDS.  ws >= cmtfpls_kfold_inner_coupled_tensor_workspace_bytes(blocks, nb, dims) (0 for bad dims).
 * cmtfpls_kfold_inner_coupled_tensor_lds_bytes (host only) returns those doubles in bytes, as the launch sizes them.  It reads A and B
 * of every view and M of the first and no buffer, so the views' pointers may be null and their other fields unset.  0 for nb outside
 * 1..8, dims that do not multiply to B, or A, B or M <= 0 alone: blocks past a limit of the entry still get their byte count.  With
 * one block of order 4 it is cmtfpls_kfold_inner_tensor_lds_bytes of that block. */
size_t cmtfpls_kfold_inner_coupled_tensor_workspace_bytes(const cmtfpls_kfold_state* blocks, int nb, const int* dims);
size_t cmtfpls_kfold_inner_coupled_tensor_lds_bytes(const cmtfpls_kfold_state* blocks, int nb, const int* dims);
int cmtfpls_kfold_inner_coupled_tensor_f64(const cmtfpls_kfold_state* blocks, int nb, const int* dims, const int* model_fold, int groups,
                                           int a, double tol, int max_iter, double* Wk, double* Wl, void* ws, size_t ws_bytes,
                                           void* stream);
/* kfold_combine_scores: out[i] = (sum_b sc[b * n + i]) / nb for i < n, the blocks added in order; 1 <= nb <= 8. */
int cmtfpls_kfold_combine_scores_f64(const double* sc, int nb, int64_t n, double* out, void* stream);

/* ---- Response-permutation test of K-fold Q2Y (validate.permutation_test_q2y) -------------------------------------------------
 * A pass carries G permuted responses x K folds = n <= 32 models in one cmtfpls_kfold_state (its K = n): model m = k G + p holds
 * out fold k = model_fold[m] and is fitted to Y[pi_p]; every model shares each read of X.  Per pass: kfold_wide_xcov (every model's
 * training cross-covariance from ONE pass over X), kfold_epilogue_grouped stage 0, then per component kfold_inner_grouped, the
 * MTTKRP X_0 WA (.) WB with n columns, kfold_epilogue_grouped stage 1, and (all but the last) the contraction X_0^T tm and stage 2.
 * The state's mean is K x A*B (per fold) and its Tout is G x I x R (group g = m % G: the held-out scores of permutation g).
 * With model_fold[m] = m and groups = 1 the grouped entries are bitwise cmtfpls_kfold_inner_f64 / cmtfpls_kfold_epilogue_f64. */
/* kfold_wide_xcov: S (K x W x A*B) = for every fold k, X_c[train_k]^T (Y'[train_k] - ydev_k) with Y' (I x W, W <= 1024 columns,
 * already centred by the all-rows mean) and ydev (K x W) the training mean of Y' per fold; the fold-grouped partials on the f64
 * matrix cores from ONE pass over X in the fold-sorted row order `order`, fold k's rows at positions fold_off[k] .. fold_off[k+1]-1.
 * Also mean (K x A*B, training column means) and stats (2 A*B: column sums and sums of squares of all rows).  Sums run in a fixed
 * order (the same bits on every run).  ws >= cmtfpls_kfold_wide_xcov_workspace_bytes(I, A * B, W, K). */
size_t cmtfpls_kfold_wide_xcov_workspace_bytes(int64_t I, int64_t P, int W, int K);
int cmtfpls_kfold_wide_xcov_f32(const float* X, int64_t I, int A, int B, const double* Y, int W, const int* order, const int* fold_off,
                                int K, const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_kfold_wide_xcov_f64(const double* X, int64_t I, int A, int B, const double* Y, int W, const int* order, const int* fold_off,
                                int K, const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream);
/* 16-bit X: as cmtfpls_kfold_xcov_bf16.  A lane's 4 columns are one 8-byte load when A * B % 4 == 0 and X is 8-byte aligned. */
int cmtfpls_kfold_wide_xcov_bf16(const uint16_t* X, int64_t I, int A, int B, const double* Y, int W, const int* order, const int* fold_off,
                                 int K, const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_kfold_wide_xcov_f16(const uint16_t* X, int64_t I, int A, int B, const double* Y, int W, const int* order, const int* fold_off,
                                int K, const double* ydev, double* S, double* mean, double* stats, void* ws, size_t ws_bytes, void* stream);
/* kfold_inner_grouped / kfold_epilogue_grouped: cmtfpls_kfold_inner_f64 / cmtfpls_kfold_epilogue_f64 for st->K = n models in
 * `groups` groups (n % groups == 0), model m holding out fold model_fold[m] (device, n entries, < n / groups). */
int cmtfpls_kfold_inner_grouped_f64(const cmtfpls_kfold_state* st, const int* model_fold, int groups, int a, double tol, int max_iter,
                                    void* ws, size_t ws_bytes, void* stream);
int cmtfpls_kfold_epilogue_grouped_f64(const cmtfpls_kfold_state* st, const int* model_fold, int groups, int stage, int a, const double* in,
                                       void* stream);
/* kfold_inner_coupled_grouped: cmtfpls_kfold_inner_coupled_f64 for the permutation test of a coupled model: `blocks` holds nb <= 8
 * views of n = K models in `groups` groups (n % groups == 0, n / groups >= 2 folds, I >= the number of folds), model m holding out
 * fold model_fold[m] (device, n entries, < n / groups).  Every view's mean is folds x A_b*B_b (what kfold_wide_xcov writes for that
 * block) and model m reads row model_fold[m] of it; S, the loadings, Q, vec, n_iter, status and Gy are per model.  Per pass:
 * kfold_wide_xcov per block (Y', ydev shared), kfold_epilogue_grouped stage 0 on blocks[0], then per component this entry, the MTTKRP
 * per block with n columns, kfold_combine_scores, kfold_epilogue_grouped stage 1 on blocks[0] and (all but the last) per block the
 * contraction and kfold_epilogue_grouped stage 2 on blocks[b]: 2R reads of each block per pass.  Same workspace
 * (cmtfpls_kfold_inner_coupled_workspace_bytes), view checks and limits as cmtfpls_kfold_inner_coupled_f64; nb, model_fold and
 * groups are checked first (CMTFPLS_EINVAL), everything on the host before anything is launched.  With model_fold[m] = m and
 * groups = 1 it is bitwise cmtfpls_kfold_inner_coupled_f64. */
int cmtfpls_kfold_inner_coupled_grouped_f64(const cmtfpls_kfold_state* blocks, int nb, const int* model_fold, int groups, int a, double tol,
                                            int max_iter, void* ws, size_t ws_bytes, void* stream);

/* ---- Repeated K-fold Q2Y (validate.get_q2y_repeated_kfold) -------------------------------------------------------------------
 * A pass carries G shuffled splits x K folds = n <= 32 models (n <= I) in one cmtfpls_kfold_state (its K = n), split-major: model
 * m = g K + k holds out fold k of split g, so each split's S, mean and Y side are a contiguous K-model slice.  Per pass:
 * cmtfpls_kfold_xcov_* once per split (one read of X each, into that split's slice), kfold_epilogue_splits stage 0, then per
 * component cmtfpls_kfold_inner_f64 (a ctPLS: cmtfpls_kfold_inner_coupled_f64 on the block views), the MTTKRP with n columns,
 * kfold_epilogue_splits stage 1, and (all but the last) the contraction X_0^T tm and stage 2.  G + 2R - 1 reads of X per pass.
 * The state's fold_of is splits x I (row g: split g's fold id of every sample, 0..K-1) and its Tout is splits x I x R (slot g:
 * split g's held-out scores, every row written once). */
/* kfold_epilogue_splits: cmtfpls_kfold_epilogue_f64 for st->K = n models in `splits` split-major splits (n % splits == 0,
 * n / splits >= 2 folds each); stage 1 trains model m on the rows with fold_of[(m / folds) I + i] != m % folds and writes its
 * held-out scores to Tout slot m / folds.  Stages 0 and 2 are those of cmtfpls_kfold_epilogue_f64; with splits = 1 the entry is
 * bitwise cmtfpls_kfold_epilogue_f64. */
int cmtfpls_kfold_epilogue_splits_f64(const cmtfpls_kfold_state* st, int splits, int stage, int a, const double* in, void* stream);

/* ---- Bootstrap of the factors (validate.bootstrap_factors) --------------------------------------------------------------------
 * A resample differs from the fitted data only in each row's multiplicity c (0, 1, 2, ..).  A pass carries n <= 32 resamples
 * (n <= I) as the models of one cmtfpls_kfold_state (its K = n), whose fold_of is n x I counts: model b trains on the rows with
 * c_b,i > 0, every training-row sum weighted by c_b,i.  Per pass: kfold_weighted_xcov (every model's S and mean from ONE pass
 * over X), kfold_epilogue_weighted stage 0, then per component cmtfpls_kfold_inner_f64 (a ctPLS: cmtfpls_kfold_inner_coupled_f64),
 * the MTTKRP with n columns, kfold_epilogue_weighted stage 1, and (all but the last) the contraction X_0^T tm and stage 2.  2R
 * reads of X per pass. */
/* kfold_weighted_xcov: S (n x M x A*B) = X_0^T (c_b * (Y - nu_b)) and mean (n x A*B) = X_0^T c_b / I for every model b from ONE
 * pass over X on the f64 matrix cores; Y (I x n (M + 1), n (M + 1) <= 1024) holds the columns c_b * (Y - nu_b) model by model,
 * then the n count columns c_b as doubles (sum_i c_b,i = I).  stats (2 A*B): column sums and sums of squares of all rows,
 * unweighted.  Sums run in a fixed order.  ws >= cmtfpls_kfold_weighted_xcov_workspace_bytes(I, A * B, n, M). */
size_t cmtfpls_kfold_weighted_xcov_workspace_bytes(int64_t I, int64_t P, int n, int M);
int cmtfpls_kfold_weighted_xcov_f32(const float* X, int64_t I, int A, int B, const double* Y, int n, int M, double* S, double* mean,
                                    double* stats, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_kfold_weighted_xcov_f64(const double* X, int64_t I, int A, int B, const double* Y, int n, int M, double* S, double* mean,
                                    double* stats, void* ws, size_t ws_bytes, void* stream);
/* 16-bit X: as cmtfpls_kfold_xcov_bf16. */
int cmtfpls_kfold_weighted_xcov_bf16(const uint16_t* X, int64_t I, int A, int B, const double* Y, int n, int M, double* S, double* mean,
                                     double* stats, void* ws, size_t ws_bytes, void* stream);
int cmtfpls_kfold_weighted_xcov_f16(const uint16_t* X, int64_t I, int A, int B, const double* Y, int n, int M, double* S, double* mean,
                                    double* stats, void* ws, size_t ws_bytes, void* stream);
/* kfold_epilogue_weighted: cmtfpls_kfold_epilogue_f64 for st->K = n weighted models (2 <= n <= I): stage 0 builds the Gram
 * sum_i c_i y_i y_i^T of each model's Yk (rows with c = 0 must be 0); stage 1 weights every training-row sum by c, writes
 * tm = c t and deflates the rows with c > 0; T keeps every row's score, the rows with c = 0 their projection (Tout is not
 * written); stage 2 is that of cmtfpls_kfold_epilogue_f64.  With 0/1 counts the entry is bitwise cmtfpls_kfold_epilogue_f64 on
 * the folds whose training rows they mark. */
int cmtfpls_kfold_epilogue_weighted_f64(const cmtfpls_kfold_state* st, int stage, int a, const double* in, void* stream);
/* ---- Nested K-fold Q2Y (validate.get_q2y_nested_kfold) ------------------------------------------------------------------------
 * The K_o (K_i + 1) models of a nested cross-validation are 0/1-weighted models of the bootstrap's pass (kfold_weighted_xcov ..
 * kfold_epilogue_weighted above), which leaves T (n x I x R: every row's score, the rows with weight 0 their projection), coef
 * (n x R x R, upper triangular) and Q (n x R x M) on the device.  press_rows scores them there:
 *   h = T[j, i, :] coef[j],   pred_r[j, i, :] = nu[j] + sum_{c < r} h_c Q[j, c, :]         (nu: n x M, the models' means of Y)
 *   press[j, r - 1] = sum over the rows i with eval[j, i] > 0 and over m of (pred_r[j, i, m] - Y[i, m])^2        (press: n x R)
 * and, where eval[j, i] == 2 and pred is not NULL, pred[r - 1, i, :] = pred_r[j, i, :] (pred: R x I x M; a row may have
 * eval == 2 in at most one model; other rows of pred are left as they are).  eval is n x I ints: 0 = the row is skipped and
 * nothing of it is read but that word.  The strictly lower triangle of coef is not read.  Sums run in a fixed order (the same
 * bits on every call).  Limits: R <= 64, M <= 64, n <= 65535 (CMTFPLS_EUNSUPPORTED otherwise, before anything is launched).
 * ws >= cmtfpls_press_rows_workspace_bytes(n, I, R, M). */
size_t cmtfpls_press_rows_workspace_bytes(int n, int64_t I, int R, int M);
int cmtfpls_press_rows_f64(const double* T, const double* coef, const double* Q, const double* nu, const double* Y, const int* eval,
                           int n, int64_t I, int R, int M, double* press, double* pred, void* ws, size_t ws_bytes, void* stream);
/* fit_small: the COMPLETE tPLS.fit (tpls.py:73-120: preprocess, every component's NIPALS loop with its convergence test,
 * rank-1 extraction, deflation, inner regression, Y deflation) of a small problem in ONE launch of one workgroup -- a fit of
 * BASELINE configs[0] (200 x 10 x 8, R = 3) is otherwise a few hundred launches of pure latency.  float64, X of order 2 or 3
 * (A = 1 for a matrix) WITHOUT missing values; limits as loo_tpls: min(A, B) <= 64, M <= 64, R <= 16, the workgroup's vectors
 * within 150 KB of LDS (CMTFPLS_EUNSUPPORTED otherwise).  Outputs (device): T (I x R), U (I x R), WA (A x R), WB (B x R),
 * Q (M x R), coef (R x R), ssq ((R + 1) x 2: row 0 = |X_c|^2, |Y_c|^2, row a + 1 = the deflated norms after component a, so
 * R2X[a] = 1 - ssq[a+1][0] / ssq[0][0] and R2Y likewise, tpls.py:115-120), x_mean (A * B), y_mean (M), n_iter (R ints),
 * flag (one int, zeroed by the caller: set to 1, nothing else written, when X or Y holds a non-finite value).
 * ws: cmtfpls_fit_small_workspace_bytes (the centred working copies of X and Y). */
size_t cmtfpls_fit_small_workspace_bytes(int I, int A, int B, int M);
int cmtfpls_fit_small_f64(const double* X, const double* Y, int I, int A, int B, int M, int R, double tol, int max_iter,
                          double* T, double* U, double* WA, double* WB, double* Q, double* coef, double* ssq, double* x_mean,
                          double* y_mean, int* n_iter, int* flag, void* ws, size_t ws_bytes, void* stream);

/* ---- synthetic inputs on the device: cmtf_pls/synthetic.py:59-74 (import_synthetic), :5-34 (make_synthetic_test)
 * The dense CP tensor of the drawn factors is cmtfpls_recon_* with T = the sample factor; add_noise then adds
 * sigma * N(0,1) in place (synthetic.py:71,74) and, if nan_fraction > 0, plants an i.i.d. NaN mask (BASELINE
 * configs[3]).  The generator is counter based (Philox4x32-10, key = seed, counter = (offset + e) / 4 for
 * element e of this buffer; offset = the buffer's first GLOBAL element index): a row shard of a
 * tensor receives exactly the noise those rows have in the whole tensor. */
int cmtfpls_add_noise_f32(float* X, int64_t n, double sigma, uint64_t seed, uint64_t offset, double nan_fraction,
                          void* stream);
int cmtfpls_add_noise_f64(double* X, int64_t n, double sigma, uint64_t seed, uint64_t offset, double nan_fraction,
                          void* stream);

/* ---- measured HBM ceilings (the roofline denominator "re-measured with a device copy
 * kernel"; not a reference call site) ---------------------------------------------------------------
 * Plain 16-byte-per-lane non-temporal streaming kernels over `bytes` of a 16-byte-aligned buffer:
 * read (sum kept in sink[0..blocks)), in-place read-modify-write (negates: two calls restore the data),
 * copy src -> dst, each under one of four workgroup -> address maps:
 *   0 flat (consecutive workgroups adjacent, grid stride; row_bytes ignored),
 *   1 chunked (a 256-thread workgroup owns row_bytes contiguous bytes at a time, grid stride over rows),
 *   2 row per 1024-thread workgroup, barrier between the read burst and the write burst (row_bytes = 16 KB * {1,2,4,8}):
 *     the map of deflate_rows / center_rows / score_deflate,
 *   3 column owner: a 256-thread workgroup owns 8 KB of columns and a block of rows, 4 rows in flight (row_bytes a
 *     multiple of 8 KB; `blocks` = total workgroups): the map of the contraction and of deflate_contract.
 * blocks <= cmtfpls_ceiling_max_blocks(). */
int cmtfpls_ceiling_max_blocks(void);
int cmtfpls_ceiling_read(const void* buf, size_t bytes, int64_t row_bytes, int map, float* sink, int blocks, void* stream);
int cmtfpls_ceiling_rmw(void* buf, size_t bytes, int64_t row_bytes, int map, int blocks, void* stream);
int cmtfpls_ceiling_copy(const void* src, void* dst, size_t bytes, int64_t row_bytes, int map, int blocks, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* CMTFPLS_H */
