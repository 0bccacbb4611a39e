/*
 * nuts_oracle.h — C interface of the CPU oracle.
 *
 * TEST INFRASTRUCTURE ONLY.  Nothing under oracle/ is part of the product: only
 * tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may load it.
 *
 * PARITY UNPINNED value for value (statistical pins on reference-held outputs: item 10 below): the algorithm this file restates lives in the crates.io
 * dependency `nuts-rs 0.18.3` (reference Cargo.toml:24, Cargo.lock:2295-2298),
 * whose source is not in /root/reference and cannot be built here (no Rust
 * toolchain, no network).  The oracle follows SURVEY.md Appendix A (a restatement
 * of the crate's published diag-NUTS algorithm) and the in-tree evidence cited
 * next to each function in nuts_oracle.cpp.  Its RNG stream is the engine's own
 * contract (include/nphip_spec.h), not nuts-rs's ChaCha8 stream, so the three
 * golden files in the reference's tests/reference/ can only be used as
 * distributional fixtures (tests/test_oracle_statistics.py).
 *
 * WHERE THIS FILE DEPARTS FROM, OR PINS DOWN, SURVEY.md APPENDIX A — each with its source.  None of these can be checked
 * against nuts-rs 0.18.3 here; they are listed so that a maintainer with the crate at hand knows what to compare first.
 *
 *  1. Divergence test is ONE-SIDED: a leapfrog diverges when energy_error > max_energy_error or is not finite
 *     (nuts_oracle.cpp Hamiltonian::leapfrog).  SURVEY A.5 / A6 write |energy_error|.  Source of the choice: the reference's
 *     own documentation of the knob — "max_energy_error: the maximum energy error ... before a divergence is declared"
 *     (docs/sampling-options.qmd:71-73) speaks of the error growing, and a large NEGATIVE error means the trajectory moved to
 *     a much more probable region, which Stan (and, from memory, nuts-rs `energy_error > max_energy_error`) does not treat as
 *     a divergence.  A two-sided test would change `diverging` only for |dH| > 1000 with dH < 0.
 *  2. Window bounds: early_end = ceil(early_window * T), final_window = T - ceil(step_size_window * T) + 1 with the
 *     comparison `draw < final_window` (Chain::Chain).  SURVEY A.8 writes final_start = ceil((1 - step_size_window) * T);
 *     the two differ by at most one draw.  Source: the crate computes `num_tune.saturating_sub(final_second_step_size)` style
 *     integer bounds (recalled); the reference only documents "the last 15 % of tuning use a fixed mass matrix"
 *     (docs/sample-stats.qmd:85, python/nutpie/sample.py:889-895).
 *  3. A mass-matrix refresh needs at least 3 draws in the estimator it reads (`n_src >= 3`, Chain::adapt): with fewer,
 *     M2_q / M2_g is 0 / 0 or a single-sample ratio.  SURVEY A.9 does not state a minimum; in-tree evidence for the formula
 *     itself: python/nutpie/normalizing_flow.py:1906-1915.
 *  4. `is_late` (`switch_freq + draw > final_window`): no estimator switch is started that could not collect switch_freq
 *     draws before the final window; the symmetric acceptance statistic drives dual averaging from then on.  SURVEY A.8 has
 *     the same condition in the form `d + freq <= final_start`.
 *  5. Welford variance is M2 / n for the gradient-based ratio (the ratio cancels the normalisation) and M2 / (n - 1) for
 *     draw_diag (Chain::adapt); SURVEY A.9 flags "n vs n-1" as unknown.
 *  6. Initial step-size search: at most 100 iterations, doubling / halving, restarted once when the first data-driven mass
 *     matrix replaces the gradient-based initial one; a divergent probe leapfrog keeps `initial_step`.
 *  7. Arithmetic FORMS shared with the engine (results identical in exact arithmetic, different rounding): tree weights as
 *     m * 2^e instead of log_size (+ logaddexp), acceptance statistic as sum / count instead of a running mean.  Setting
 *     `crate_arithmetic = 1` uses the crate's forms instead; the decisions (depth, n_steps, index_in_trajectory) of both
 *     modes are compared on the golden cases in tests/test_oracle_kat.py.
 *  8. RNG: Philox4x32-10 counter streams keyed by (seed, global chain, draw, purpose) and Box-Muller normals instead of the
 *     crate's ChaCha8 + ziggurat; summation in the engine's fixed order (`waves_per_chain`).  By construction, not by
 *     evidence: the crate's stream cannot be reproduced without the crate.
 * 10. WHAT THE REFERENCE-HELD NUMBERS SAY ABOUT ALL THIS (round 5; scratch/r5_reference_sensitivity.py -> profiles/r5_reference_sensitivity.txt,
 *     asserted by tests/test_oracle_reference_pins.py and, for the engine, tests/test_gpu_reference_fixtures.py).  Value-for-value
 *     parity stays unpinned (the crate's RNG stream), but two bodies of evidence in the reference's tree are outputs of nuts-rs:
 *     (a) the FINAL step sizes and last-draw gradient counts of 36 chains in the frozen docs (docs/_freeze; three analytic models,
 *         default settings; tests/golden/reference_doc_step_sizes.json).  The restatement reproduces them: z = +0.7 / +0.5 / +0.1 for the
 *         three models' means (KS p 0.36 / 0.42 / 0.90), the same non-power-of-two gradient counts (9, 11, 13, 19, 27: a doubling
 *         stops inside the sub-tree that turns) with the same mean.  These numbers REJECT: plain instead of symmetric acceptance
 *         in the late windows (z = +4.7), target_accept 0.75 / 0.85 (z = -10 / +13), dual-averaging gamma 0.1 (z = -7), the last
 *         tuning draw keeping its step instead of step_size_bar (spread x 8).  They cannot tell apart: early_window 0.3 / 0.5,
 *         step_size_window 0.10 / 0.15, switch frequencies 10 / 20 and 80 / 50, a refresh from 1 / 3 / 10 draws (departure 3), when
 *         the step-size search runs (departure 6), truncated window bounds (departure 2), t0, k.
 *         Two more runs of the same docs (docs/sample-stats.qmd, tune 1000): Neal's funnel — step 0.403 +- 0.074 against 0.442 +- 0.055 (z = -1.7), divergence
 *         counts inside this sampler's per-chain distribution — and a 102-dimensional Gaussian with one direction stiffer by 1e4 — step 0.158 +- 0.032
 *         against 0.155 +- 0.028 (z = +0.3), 31 gradients in five last draws of six against P(31) = 0.91 here, no divergence on either side: the adapted
 *         sampler's step size AND tree depth in 102 dimensions (this model also leans against a main-phase switch frequency of 50: z = -2.3; 80: +0.2).
 *         48 chains of nuts-rs on five models in all; and the bulk ESS the docs print for one of them (1517 of 6000 draws) at rank 0.67 of 100 runs here.
 *     (b) the HalfNormal files.  Stan flavour (2 x 10 draws): every statistic between ranks 0.29 and 0.78 of 2000 runs of its shape.
 *         PyMC flavour (2 x 100 draws): lag-1 autocorrelation 0.993, repeat fraction 0.04, deepest excursion (min log a = -8.1)
 *         0.017 — inside the 0.5 - 99.5 % band —, but pooled mean 0.560 and median 0.375 at rank 0.0015, and NO variant of the
 *         recalled constants above, nor PyMC's initial points instead of U(-2, 2), moves them (0.0000 - 0.0065 across the 17
 *         variants); conditional on an excursion as deep as the file's (1.8 % of runs) they stay at 0.000 - 0.003.  The reference's CHANGELOG.md:124 ("Update
 *         reference draws due to change in window lengths") says the files were regenerated for window lengths that may differ from the recalled
 *         ones: an 81-point grid over the four window constants (profiles/r5_window_grid.txt) leaves both ranks at <= 0.005 everywhere.  The file spends
 *         half of its 200 draws below a = 0.375 in three separate excursions to the left tail; this sampler's runs of that shape do
 *         not.  OPEN: either a 1-in-500 realisation or a difference that none of the recalled knobs expresses.
 *  9. `step_size_adapt_method = "adam"` (Adam on log step size, src/wrapper.rs:344-376): beta1 0.9, beta2 0.999, eps 1e-8 are
 *     the textbook constants; the crate's are unknown.  SURVEY §2 marks the option out of scope; it is kept only because
 *     the settings surface accepts the value.
 */
#ifndef NUTS_ORACLE_H
#define NUTS_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Same signature as the reference's raw C logp callback (src/pymc.rs:23-29,
 * python/nutpie/compile_pymc.py:975-981): 0 ok, >0 recoverable, <0 fatal. */
typedef int64_t (*oracle_logp_fn)(uint64_t dim, const double* x, double* grad, double* logp, void* user);

typedef struct {
    /* DiagNutsSettings (reference src/wrapper.rs:525-533, 563-620, 213-447) */
    uint64_t seed;
    uint64_t num_tune;
    uint64_t num_draws;
    uint64_t num_chains;
    uint64_t maxdepth;
    uint64_t mindepth;
    int32_t check_turning;
    int32_t use_grad_based_mass_matrix;
    double max_energy_error;
    /* adapt_options */
    double early_window;
    double step_size_window;
    uint64_t mass_matrix_switch_freq;
    uint64_t early_mass_matrix_switch_freq;
    uint64_t mass_matrix_update_freq;
    /* step_size_settings */
    double initial_step;
    double target_accept;
    double step_size_jitter;   /* 0 => none */
    double max_step_size;
    double da_k, da_t0, da_gamma;
    int32_t fixed_step_size;   /* !=0: step_size_adapt_method = "<float>" */
    int32_t adapt_mass_matrix; /* 0: keep the initial (identity/explicit) matrix; test knob */
    /* init */
    int32_t init_kind;         /* 0: U(-2,2) (src/pyfunc.rs:540-544)  1: N(0,1) (src/stan.rs:798-808)  2: explicit */
    int32_t num_try_init;
    /* engine geometry */
    int32_t waves_per_chain;
    int32_t n_threads;
    /* global chain id of local chain 0 (multi-GPU sharding invariance) */
    uint64_t chain_offset;
    /* optional outputs */
    int32_t store_gradient;
    int32_t store_mass_matrix;
    /* step_size_adapt_method = "adam" (src/wrapper.rs:344-376, 391-407): Adam on log(step size) */
    int32_t adam;
    /* 0 (default): the arithmetic FORMS the engine uses — tree weights m * 2^e, acceptance statistics as sum / count.
     * bit 0: tree weights in the crate's form — log_size merged with logaddexp, accepted with exp(log_size_other - self_w)
     *        (SURVEY.md App. A.3 verbatim).  Same uniforms; every float and decision of the golden cases is unchanged.
     * bit 1: the acceptance statistic as an incrementally updated running mean (App. A.6 verbatim).  Differs from sum / count
     *        in the last bits; through dual averaging that perturbs the step size by ~1e-16 relative, and a chaotic
     *        integrator amplifies it until some U-turn test flips: identical decisions on four golden cases, a fork at
     *        draw 36 of the fifth.  tests/test_oracle_kat.py pins both statements. */
    int32_t crate_arithmetic;
    double adam_learning_rate;
    int32_t store_divergences;
    /* Low-rank metric M^-1 = D^1/2 (I + V (Lambda - I) V') D^1/2 (adaptation="low_rank": src/wrapper.rs:307-334,
     * python/nutpie/sample.py:921-933).  The ESTIMATOR of (sigma^2, V, lambda) is not part of the oracle (it lives in
     * nutpie_amd/low_rank.py and follows the published description); what the oracle restates is the sampler UNDER such a
     * metric, with the metrics handed in: update u replaces the metric of every chain before draw metric_draws[u]
     * (sigma2[u][chain][dim], V[u][chain][k][dim] — row j = column j of V —, lambda[u][chain][k]); the chain keeps its
     * position, re-runs the step-size search and stops adapting its own diagonal.  low_rank_metric = 0: plain diag-NUTS. */
    int32_t low_rank_metric;
    int32_t n_metric_updates;
    int32_t metric_k;
    uint64_t metric_draws[16];
    const double* metric_sig2;
    const double* metric_V;
    const double* metric_lam;
} oracle_settings_t;

typedef struct {
    /* all arrays [chains][T] (T = num_tune + num_draws) unless noted */
    double* draws;            /* [chains][T][dim] */
    int64_t* depth;
    int64_t* n_steps;
    int64_t* index_in_trajectory;
    uint8_t* diverging;
    uint8_t* maxdepth_reached;
    uint8_t* tuning;
    double* energy;
    double* energy_error;
    double* logp;
    double* step_size;
    double* step_size_bar;
    double* mean_tree_accept;
    double* mean_tree_accept_sym;
    double* gradient;         /* [chains][T][dim] or NULL */
    double* mass_matrix_inv;  /* [chains][T][dim] or NULL */
    /* store_divergences (python/nutpie/sample.py:631-650): all four [chains][T][dim] or all NULL; rows of draws that did not
     * diverge are NaN; divergence_end is NaN too when the divergence was a logp error rather than an energy error */
    double* divergence_start;
    double* divergence_end;
    double* divergence_momentum;
    double* divergence_start_gradient;
} oracle_trace_t;

void oracle_default_settings(oracle_settings_t* s);

/* Tridiagonal-precision Gaussian  logp(x) = -1/2 (x-mu)' L (x-mu),
 * L = tridiag(offdiag, diag, offdiag).  mu may be NULL (zero), offdiag may be NULL. */
int oracle_sample_tridiag(const oracle_settings_t* s, uint64_t dim, const double* mu, const double* diag,
                          const double* offdiag, const double* init_points, oracle_trace_t* out, double* seconds);

/* Arbitrary host callback model. */
int oracle_sample_callback(const oracle_settings_t* s, uint64_t dim, oracle_logp_fn fn, void* user,
                           const double* init_points, oracle_trace_t* out, double* seconds);

const char* oracle_last_error(void);

/* Experiment knobs for the sensitivity study of the reference-held evidence (scratch/r5_reference_sensitivity.py): which of the
 * recalled details of the crate's warm-up the oracle follows.  Defaults (3, 2, 1, 1, 0) = the restatement every parity test runs. */
void oracle_set_variant(int min_refresh, int search_mode, int late_sym, int last_bar, int floor_windows);

/* ---- unit-level entry points for known-answer tests ---- */
void oracle_philox(uint64_t seed, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t out[4]);
void oracle_detmath(int fn, uint64_t n, const double* x, double* y); /* 0 exp 1 log 2 log1p 3 sin2pi 4 cos2pi */
double oracle_logaddexp(double a, double b);
/* every function of the contract on records x[n][n_in] -> y[n][n_out]: the fn codes and record shapes of nphip_test_spec (include/nutpie_hip.h: exp_parts,
 * w_rel, logaddexp, the normal pair of four given words, Philox words, ...); 0, or -1 for an unknown fn or a wrong shape */
int oracle_spec(int fn, uint64_t n, int n_in, const double* x, int n_out, double* y);
void oracle_w_leaf(double neg_energy_error, double* m, int64_t* e);
void oracle_w_add(double m1, int64_t e1, double m2, int64_t e2, double* m, int64_t* e);
void oracle_normals(uint64_t seed, uint32_t chain, uint32_t draw, uint32_t purpose, uint64_t n, double* out);
/* Dense-precision Gaussian logp(x) = -1/2 (x-mu)' P (x-mu) with the engine's gradient summation order (nutpie_amd/csrc/dense_tile.h,
 * include/nphip_spec.h "dense gradient"): the oracle counterpart of nphip_model_dense_gaussian.  P [dim][dim] row-major, borrowed. */
int oracle_sample_dense(const oracle_settings_t* s, uint64_t dim, const double* mu, const double* P, const double* init_points,
                        oracle_trace_t* out, double* seconds);
void oracle_dense_grad(uint64_t n, uint64_t dim, const double* x, const double* mu, const double* P, int waves, double* grad, double* logp);
double oracle_dot(const double* x, const double* y, uint64_t n, int waves);
/* one leapfrog on the tridiag model; state arrays are in/out. returns energy U'+K'. */
double oracle_leapfrog_tridiag(uint64_t dim, const double* mu, const double* diag, const double* offdiag,
                               const double* sig2, double eps, int waves, double* q, double* p, double* g,
                               double* kinetic, double* potential);
/* dual averaging trajectory: feeds accept[i], writes step_size[i], step_size_bar[i] after each advance */
void oracle_dual_average(double initial_step, double target, double k, double t0, double gamma, uint64_t n,
                         const double* accept, double* step, double* step_bar);
/* Welford running variance over n samples of dimension dim: outputs mean, M2 */
void oracle_welford(uint64_t n, uint64_t dim, const double* samples, double* mean, double* m2);
/* v = M^-1 p under the low-rank metric (k rows of V, each of length dim) */
void oracle_lr_velocity(uint64_t dim, int k, const double* sig2, const double* V, const double* lam, int waves, const double* p, double* v);
/* U-turn criterion on two trajectory points */
int oracle_is_turning(uint64_t dim, const double* sig2, int waves, int64_t idx1, const double* p1,
                      const double* psum1, int64_t idx2, const double* p2, const double* psum2);

/* ---- the order contracts of the stages inside the generated densities (nutpie_amd/csrc/chain_scan.h, chain_matvec.h, chain_linalg.h;
 * DESIGN.md 11.5-11.7), restated from their text; the device routines are compared with these bit for bit ---- */
/* x_t = a_t x_{t-1} + b_t on R rows of T elements as W waves per chain compute it.  a_kind: 0 an array a[R T], 1 the scalar a_s, 2 the
 * constant 1 (plain additions).  rev: the adjoint lambda_t = a_{t+1} lambda_{t+1} + b_t.  init[R] when init_per_row, else i_s. */
void oracle_chain_scan(int R, int T, int W, int a_kind, int rev, int init_per_row, const double* a, double a_s, const double* b,
                       const double* init, double i_s, double* x);
/* E[n][R] = X B (Xt[K][n] the transposed matrix, B[K][R]);  C[K][R] = X^T G (X[n][K], G[n][R]) */
void oracle_chain_times(int n, int K, int R, const double* Xt, const double* B, double* E);
void oracle_chain_times_t(int n, int K, int R, const double* X, const double* G, double* C);
/* K x K row-major.  cholesky: returns 1, or 0 with all of L NaN when a pivot is not positive and finite; the upper triangle is +0.0 */
int oracle_chain_cholesky(int K, const double* A, double* L);
void oracle_chain_solve_lower(int K, int N, const double* L, const double* B, double* X);
/* Y = L^-T G on a block whose element (i, c) is at i rs + c cs (G and Y may be the same array) */
void oracle_chain_solve_lower_t(int K, int N, int rs, int cs, const double* L, const double* G, double* Y);
void oracle_chain_solve_lower_adj_l(int K, int N, const double* Bbar, const double* X, double* Lbar);
void oracle_chain_cholesky_adj(int K, const double* L, const double* Lbar, double* Abar);

#ifdef __cplusplus
}
#endif
#endif
