"""`EngineOptions`: which exact form of each step the engine takes where the shape allows it (one object per engine)."""
from __future__ import annotations

from dataclasses import dataclass, replace
from typing import Optional


@dataclass(frozen=True)
class EngineOptions:
    """Which exact form of each step the engine takes WHERE THE SHAPE ALLOWS IT.  Every default is the fastest form; each
    switch selects the slower equivalent form the tests compare it with.  One object per engine (`NipalsEngine(backend,
    comm, options)`, `tPLS(..., options=EngineOptions(...))`); what actually ran is written to `FitState.report`
    (`tPLS.fit_report_`), so a path the shape declined is visible instead of silent."""
    # a single small float64 block without missing values: the whole fit in ONE launch (cmtfpls_fit_small_f64); a regular
    # iteration is ~20 launches of pure latency whatever the size, a one-workgroup iteration costs time in proportion to I * P
    small_fit: bool = True
    small_fit_elements: int = 1 << 15    # measured (profiles/r03q_small_fit.txt): 2.2x faster at 16000 elements, slower from 65536 on
    # algorithm="xcov" on blocks without missing values: never deflate X in place (two reads per component instead of a
    # read and a read + write, FitRun._finish_xcov_nowrite); False keeps the deflating form
    xcov_nowrite: bool = True
    # ... and, when X is never written anyway, do not centre it either: the fit runs on the caller's UNCENTRED tensor -- no
    # centring pass, no private copy -- with two rank-one corrections; False keeps the centred copy
    xcov_raw: bool = True
    # the uncentred form works by cancellation: its error grows with max|column mean| / rms spread of the centred data.
    # Beyond this ratio the fit falls back to the centred private copy (report: raw = False, raw_declined = ratio)
    xcov_raw_max_offset: float = 1e4
    # the same cancellation in transform / predict: the one-pass MTTKRP on the caller's UNCENTRED rows subtracts mean^T W
    # from X W.  Beyond this ratio (estimated from <= 256 rows of the batch) the rows are centred first: in registers where
    # the shape allows it, else on private copies (projection_report_: offset_ratio and why)
    project_raw_max_offset: float = 1e4
    # the largest block: score and the contraction with the (block-averaged) score from ONE read of it, the second read per
    # component replaced by a P x a matrix-vector product; False keeps the two reads
    xcov_one_read: bool = True
    # blocks WITH missing values, 2 M <= 64: S = X0^T Y and S2 = X0^T (Y * rowscale) from one matrix-core pass with the
    # I x 2M right-hand side [Y, Y * rowscale]; False builds them one after the other
    xcov_pair_build: bool = True
    # a fit on the uncentred tensor: |X - X_mean|^2 from the read that builds S for the first component instead of a read of
    # its own (backend.xcov_ssq); False keeps the separate pass
    xcov_ssq_with_s: bool = True
    # ... and the statistics pass too: column sums and sums of squares from the read that builds S for the first component
    # (backend.xcov_stats): a fit on the uncentred tensor reads X once before its first component; False keeps colstats first
    xcov_stats_with_s: bool = True
    # one block WITH missing values: the deflation happens inside the rebuild of S for the next component (one read + write
    # of X instead of a read + write and a read, FitRun._finish_xcov_masked_fused); False keeps the two passes
    xcov_deflate_build: bool = True
    # the inner loop on S: iteration it + 1 is ENQUEUED before the host has seen iteration it's convergence norm, into a
    # second set of buffers (FitRun._inner_loop_xcov_pipelined); False waits after every iteration
    xcov_pipeline: bool = True
    # sharded direct loop under graph replay: capture the two per-iteration all-reduces INSIDE the iteration's HIP graph (one
    # replay per iteration instead of three segments and two eager collectives); falls back to the segment-wise form when
    # the capture fails (report: collectives_in_graph)
    capture_collectives: bool = False
    # transform / predict of samples with missing values: rows WITHOUT a missing value keep the one-pass MTTKRP result and
    # only the affected rows take the masked sequential form; False runs the sequential form on every row of such a batch
    project_split_rows: bool = True
    # cross-validation of a tPLS whose X has missing values with the reference's masked arithmetic, a workgroup per model instead
    # of one regular-engine refit per model: leave-one-out and K-fold Q2Y (every fold in ONE launch, cmtfpls_cv_masked_f64,
    # kfold.masked_predictions), and the permutation test, repeated K-fold and the bootstrap (every permutation x fold, split x
    # fold or resample as a count-weighted model, cmtfpls_cv_masked_models_f64, kfold.masked_models); opt-in (reports:
    # q2y_report_ / bootstrap_report_, a decline names its reason)
    masked_folds: bool = False
    # the same for a ctPLS with a missing value in at least one block: every fold, permutation x fold, split x fold or resample as
    # a count-weighted model of all blocks with the reference's per-block masked arithmetic, a workgroup per model
    # (cmtfpls_cv_masked_coupled_f64, kfold.masked_models_coupled): K-fold / leave-one-out Q2Y, the permutation test, repeated
    # K-fold and the bootstrap; opt-in, and separate from masked_folds, under which a ctPLS keeps its refit routing
    masked_folds_coupled: bool = False
    # the permutation test of a ctPLS on complete data on the device: G permutations x K folds per pass share each read of every
    # block (cmtfpls_kfold_wide_xcov_* per block, cmtfpls_kfold_inner_coupled_grouped_f64, permutation._device_null)
    # instead of one regular-engine refit per fold and permutation; opt-in (report: q2y_report_, a decline names its reason)
    coupled_permutations: bool = False
    # cross-validation of a tPLS whose X has order 4 (I x A x B1 x B2) on the device: K-fold, the permutation test, repeated and
    # nested K-fold take it as I x A x B1 B2 with the Kronecker loading wK (x) wL, and the rank-1 CP of each fold's A x B1 x B2
    # cross-covariance runs inside the fold's workgroup (cmtfpls_kfold_inner_tensor_f64) instead of one regular-engine
    # refit per model; leave-one-out (get_q2y, loo_predictions) takes cmtfpls_loo_xcov_tensor_f64, a workgroup per fold with the
    # same CP inside, and bootstrap_factors runs its resamples through the weighted passes with the tensor inner entry, every
    # model's wK and wL coming back for the per-mode stacks; opt-in (report: q2y_report_ / bootstrap_report_ with
    # "rank1", a decline names its reason)
    tensor_folds: bool = False
    # the same for a ctPLS on complete data with at least one block of order 4 among blocks of order 2, 3 and 4: K-fold, repeated and
    # nested K-fold (and, together with coupled_permutations, the permutation test) run the coupled passes with the rank-1 CP of
    # every order-4 block's cross-covariance inside the fold's workgroup (cmtfpls_kfold_inner_coupled_tensor_f64);
    # opt-in, and separate from tensor_folds, under which a ctPLS keeps its refit routing (report: q2y_report_ with "rank1")
    tensor_folds_coupled: bool = False
    # cross-validation of a tPLS whose X has order 4 AND missing values: the masked workgroup-per-model refits of masked_folds on
    # the I x A x B1 B2 view with the rank-1 CP of each model's A x B1 x B2 contraction inside its workgroup
    # (cmtfpls_cv_masked_tensor_f64, cmtfpls_cv_masked_tensor_models_f64): leave-one-out and K-fold Q2Y, the permutation
    # test, repeated K-fold and the bootstrap; opt-in, and separate from masked_folds and tensor_folds, each of which alone leaves
    # such an X to the refits (report: q2y_report_ / bootstrap_report_ with "rank1", a decline names its reason)
    masked_tensor_folds: bool = False
    # leave-one-out Q2Y (get_q2y, loo_predictions) and the factor bootstrap of a ctPLS on complete data with at least one block of
    # order 4 among blocks of order 2, 3 and 4 on the device: every fold a workgroup on the cross-covariances of the coupled blocks
    # with the rank-1 CP of every order-4 block inside it (cmtfpls_loo_xcov_coupled_tensor_f64), and the bootstrap's weighted passes
    # through cmtfpls_kfold_inner_coupled_tensor_f64 with per-mode stacks [wA, wK, wL]; opt-in, and separate from
    # tensor_folds_coupled, tensor_folds and masked_folds_coupled, each of which alone leaves these two routines on their refits
    # (report: q2y_report_ / bootstrap_report_ with "rank1", a decline names its reason)
    tensor_resamples_coupled: bool = False
    # cross-validation of a ctPLS with at least one block of order 4 (among blocks of order 2, 3 and 4) AND a missing value in at least
    # one block, of any order: the masked workgroup-per-model refits of masked_folds_coupled with every order-4 block on its
    # I x A x B1 B2 view and the rank-1 CP of its contraction inside the model's workgroup (cmtfpls_cv_masked_coupled_tensor_f64,
    # kfold.masked_models_coupled): leave-one-out and K-fold Q2Y, the permutation test, repeated K-fold and the bootstrap
    # (per-mode stacks [wA, wK, wL]); opt-in, and separate from masked_folds_coupled, which alone declines such a model to the refits
    # (report: q2y_report_ / bootstrap_report_ with "rank1", a decline names its reason)
    masked_tensor_folds_coupled: bool = False
    # cross-validation and the bootstrap of a model with 16-bit storage (dtype="bfloat16" / "float16") on the 16-bit tensor itself:
    # the complete-data device passes of K-fold, the permutation test, repeated and nested K-fold and bootstrap_factors (tPLS and
    # ctPLS, order-4 blocks under tensor_folds / tensor_folds_coupled / tensor_resamples_coupled included) read X through
    # cmtfpls_kfold_xcov_* / kfold_wide_xcov_* / kfold_weighted_xcov_*, cmtfpls_mttkrp_* and cmtfpls_xcov_* in their _bf16 / _f16
    # forms -- a caller's 16-bit device tensor is never copied -- instead of an exact float32 upcast of twice its size (DESIGN 8w,
    # "Resampling"); the float32 model's arithmetic in another f64 summation order, so not bit-identical to the upcast route.
    # Leave-one-out, the masked routes and a backend without the entries still upcast; opt-in (report: q2y_report_ /
    # bootstrap_report_ with "half_storage", else "storage_fallback" with the reason)
    half_folds: bool = False
    # the read-only diagnostics of a model with 16-bit storage on the 16-bit tensor itself: sample_diagnostics (its training-statistics
    # pass included), sample_contributions, selectivity_ratio, R2X_literal and the engine's one-read norm (tPLS and ctPLS, blocks of
    # order >= 4 on their I x A x B view) read the training tensor, or a new X that already is a device tensor of the storage type,
    # through cmtfpls_resid_rows_* / contrib_rows_* / selectivity_cols_* / recon_r2_* in their _bf16 / _f16 forms -- never copied --
    # instead of an exact float32 upcast of twice its size ("Diagnostics"); the f32 entry's thread-to-column mapping, so
    # every result has the bits of the upcast route.  A block whose kernel declines the shape (R > 16, the LDS bound of
    # contrib_rows), impute, get_q2x_heldout and a backend without the entries still upcast; opt-in (report: diagnostics_report_ /
    # contributions_report_ / importance_report_ / r2x_literal_report_ with "half_storage", else "storage_fallback" with the reason)
    half_diagnostics: bool = False
    # sparse loadings (tPLS / ctPLS `sparsity`): the soft-thresholded sweeps of an order-3 block's extraction stop when
    # max(|a - wA|_inf, |b - wB|_inf) < sparse_tol, or after sparse_max_sweeps with the last iterate kept (counted in
    # fit_report_["sparse"]["unconverged"]); a dense model reads neither
    sparse_tol: float = 1e-10
    sparse_max_sweeps: int = 200

    def but(self, **changes) -> "EngineOptions":
        return replace(self, **changes)


_DEFAULT_OPTIONS = EngineOptions()


def default_options() -> EngineOptions:
    """The options of an engine constructed without any (the product default: `EngineOptions()`)."""
    return _DEFAULT_OPTIONS


def set_default_options(options: Optional[EngineOptions]) -> EngineOptions:
    """Replace the process-wide default (None restores `EngineOptions()`); returns the previous one.  The test harness uses it
    to keep the small float64 fits of the kernel suites on the multi-launch engine (tests/conftest.py)."""
    global _DEFAULT_OPTIONS
    old, _DEFAULT_OPTIONS = _DEFAULT_OPTIONS, (options if options is not None else EngineOptions())
    return old
