/*
 * epipf.h -- C ABI of the MI355X particle-filter engine (libepipf.so).
 *
 * The reference (GeorgeEfstathiadis/Stochastic-Epidemic-Modelling) is pure Python and has no FFI;
 * its seams are plain Python calls.  These entry points replace, one for one:
 *
 *   epipf_run            pmcmc.py:123-233  particle_filter(Y, type_model, theta_proposal, observations,
 *                                          probs, n_particles, n_population, mu, jobs)
 *                        -- batched over independent chains; the per-particle joblib dispatch of
 *                           pmcmc.py:200-220 becomes one GPU lane per particle.
 *   epipf_copy_history   pmcmc.py:151-152,233  the hidden_process [T,N,C] / ancestry_matrix [T,N] outputs
 *   epipf_path_sample    pmcmc.py:236-248  particle_path_sampler(hidden_process, ancestry_matrix)
 *                        (the uniform pick np.random.randint(0, N) stays on the host RNG: `chosen`)
 *   epipf_simulate       gillespie_algo.py:10-75 / 78-146 / 148-233  sir_simulate / seir_simulate /
 *                        sir_subgroups_simulate(..., last_values_only=True), batched over states
 *   epipf_simulate_path  the same functions with last_values_only=False (event times + states)
 *   epipf_forecast       tests/pred_tmps.py:55-64  traj_inf per posterior draw (own theta, own start state), batched:
 *                        the continuous path over [0, H] binned to one row per day, with ensemble sums and histograms
 *   epipf_forecast_summary   no reference counterpart: peak, peak time, extinction time, infections and events of each
 *                        of epipf_forecast's continuous paths, reduced on the device
 *   epipf_smooth / epipf_smooth_history   no reference counterpart: the smoothing distribution over the observed window
 *                        (daily means, quantiles, surviving lineages) from the resident history, or from a caller's
 *   epipf_smooth_lag / epipf_smooth_lag_history   no reference counterpart: the fixed-lag smoother, each day from the
 *                        particles `lag` days later traced back (lag 1: the filtering distribution)
 *   epipf_resample       pmcmc.py:185-190  normalise + np.random.choice(range(N), N, p=w/sum(w)) with
 *                        caller-supplied uniforms (bit-exact to numpy's legacy choice)
 *   epipf_abc            abc_algo.py:17-109  abc_algo(observed_data, no_of_samples, threshold, priors)
 *                        -- the rejection loop batched: one GPU lane per trial, trials accepted in trial order
 *   epipf_abc_trials     abc_algo.py:33-94  one pass of the while-loop body per trial (prior draw, initial
 *                        counts, sir_simulate(..., False), daily table, distance_function) for trials [t0, t0+n)
 *   epipf_abc_smc_generation / epipf_abc_smc_weights   no reference counterpart: ABC-SMC over the same trials, one
 *                        generation (proposals from the previous weighted population) and its weight denominators
 *   epipf_if2            no reference counterpart (its PMCMC scripts start from hand-tuned runs): iterated filtering, a
 *                        maximum-likelihood search by filters whose particles each carry and jitter their own theta
 *   epipf_iterated_filtering_subgroups   the same search for the subgroup models at G = 2..4 (theta = beta[G][G], gamma)
 *   epipf_walk_filter / epipf_walk_history / epipf_walk_smooth / epipf_walk_smooth_history   no reference counterpart:
 *                        time-varying rates -- the filter of "theta follows a reflected random walk" with every day's
 *                        parameters kept, and smoothed daily beta, gamma and R_t as mean and quantiles
 *   epipf_run_incidence  no reference counterpart: the filter on reported case counts (new infections, onsets, removals
 *                        per day, with gaps and cumulated reports) instead of the compartments themselves
 *   epipf_incidence_walk / epipf_incidence_smooth   no reference counterpart: R_t from case counts -- the random-walk
 *                        filter weighted by those reports, and the smoothed true flows per day of an incidence pass
 *
 * The host wrapper (stochastic-epidemic-modelling_amd/epipf/) binds these with ctypes and keeps
 * the reference's Python signatures.  Conventions:
 *   - all pointers are HOST pointers to C-contiguous arrays owned by the caller; the context owns and
 *     reuses every device buffer (observations and history stay resident in HBM across calls);
 *   - return value 0 = EPIPF_OK, negative = error (message via epipf_last_error()); nothing throws;
 *   - one context per device; calls on one context must be serialised by the caller;
 *   - random numbers come from the keyed Philox4x32-10 stream documented in DESIGN.md §3
 *     (key = 64-bit seed per chain, filter_index = one per particle-filter call).
 */
#ifndef EPIPF_H
#define EPIPF_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EPIPF_ABI_VERSION 9

/* return codes */
#define EPIPF_OK 0
#define EPIPF_EINVAL (-1)   /* bad argument / shape */
#define EPIPF_EHIP (-2)     /* HIP runtime error */
#define EPIPF_ENOMEM (-3)   /* device allocation failed */
#define EPIPF_ESTATE (-4)   /* call order (e.g. path sample before any run) */

/* per-chain status written by epipf_run */
#define EPIPF_STATUS_OK 0
#define EPIPF_STATUS_DEGENERATE 1 /* all weights 0 or NaN at some step: reference returns (None, None, None) */
#define EPIPF_STATUS_SKIPPED 2    /* chain was inactive in this call (active[c] == 0) */

/* models: pmcmc.py:116-120 ModelType */
#define EPIPF_SIR 0
#define EPIPF_SEIR 1
#define EPIPF_SIR_SUBGROUPS 2
#define EPIPF_SIR_SUBGROUPS2 3

/* observation models: pmcmc.py:178-181 (observations=False / True) */
#define EPIPF_OBS_BINOMIAL 0
#define EPIPF_OBS_NORMAL 1
#define EPIPF_OBS_NEGBIN 2 /* the incidence filters alone, through their *_negbin entry points */

/* resampling: multinomial is the reference's (pmcmc.py:188); systematic is opt-in and changes results */
#define EPIPF_RESAMPLE_MULTINOMIAL 0
#define EPIPF_RESAMPLE_SYSTEMATIC 1

typedef struct epipf_ctx epipf_ctx;

typedef struct {
    double step_ms;              /* HIP-event time of the fused resample+propagate+weight kernels (profiling on) */
    int64_t step_launches;       /* number of such launches timed */
    double init_ms;              /* HIP-event time of the init kernels (profiling on) */
    int64_t init_launches;
    int64_t events;              /* accepted Gillespie events (profiling on) */
    int64_t particle_steps;      /* N x T_obs x chains that ran a filter */
    int64_t filters;             /* chain-filters run */
    int64_t resample_fallbacks;  /* draws resolved by the sequential bit-exact path */
    int64_t lane_iterations;     /* SSA loop iterations summed over lanes (profiling on) */
    int64_t wave_lane_slots;     /* SSA loop iterations x 64 summed over waves: lane_iterations / this = SIMD lane use */
    double abc_ms;               /* HIP-event time of the ABC trial kernels (profiling on) */
    int64_t abc_launches;        /* ABC trial kernel launches */
    int64_t abc_trials;          /* ABC trials simulated (accepted or not) */
    int64_t ssa_exact_lanes;     /* particle-steps of a filter or of iterated filtering (epipf_if2) simulated on the exact
                                    f64 SSA loop (profiling counters) */
    int64_t ssa_exact_waves;     /* wave-steps of either with at least one such particle-step */
    double step_kernel_ms;       /* summed span of each chain group's back-to-back step kernels, HIP events on the
                                    group's own stream (profiling on) */
    int64_t step_kernel_launches;/* their number: one step of all chains (step_ms) is one launch per chain group on
                                    concurrent streams (EPIPF_STREAMS, default 4) */
    int64_t last_lanes;          /* SSA lanes per particle of the last epipf_run (1: one-lane step kernel; 2..16: the
                                    lane-group step kernel, epipf_set_lanes) */
    int64_t last_lane_events;    /* events per lane per chunk of that run's lane-group kernel (1 for the one-lane one) */
    int64_t resample_ref_ambiguous; /* resampling draws whose uniform lies so close to a CDF boundary that scipy's own
                                       weights (within the measured envelope of their error) could pick
                                       a neighbouring ancestor: a diagnostic count, always on; the draw itself is the
                                       numpy answer over the device's weights */
    int64_t last_fused;          /* 1: the last epipf_run ran each chain's whole filter in one workgroup launch (N <= 512
                                    with the lanes automatic); 0: one launch per filter step */
} epipf_stats;

/* groups: G for the subgroup models (1 <= G <= epipf_max_groups() = 8), ignored (1) for SIR/SEIR.  G = 5..8 run one
 * lane per particle at every size (the lane-group and one-workgroup kernels exist for G <= 4).
 * t_max: largest T (observation rows) a run may use; max_chains: largest batch of independent filters. */
int epipf_create(epipf_ctx** out, int device, int model, int groups, int n_particles, int t_max,
                 int max_chains);
void epipf_destroy(epipf_ctx* ctx);

/* Y: [T*K] row-major observed counts (K = C, or 3 for SIR_SUBGROUPS2).  Uploaded once, kept in HBM. */
int epipf_set_observations(epipf_ctx* ctx, const double* Y, int T, int K);

/* n_population, mu: [G] (pmcmc.py:129-131; G = 1 for SIR/SEIR).  n_population must be integral. */
int epipf_set_population(epipf_ctx* ctx, const double* n_population, const double* mu);

/* Run n_chains independent particle filters (one per chain) over the resident observations.
 *   theta  [n_chains*d]: SIR (beta, gamma); SEIR (beta, alpha, gamma); subgroups beta[G][G] row-major + gamma
 *   probs  [n_chains]   : binomial detection probability, or the normal-noise ratio (observations=True)
 *   keys   [n_chains]   : Philox key per chain;  filter_index [n_chains]: stream index of this call
 *   active [n_chains] or NULL: 0 marks a chain that runs nothing this call (status SKIPPED)
 *   log_zetas_out [n_chains*T] or NULL: log of the reference's zetas (zetas = exp(log_zetas))
 *   status_out [n_chains]: EPIPF_STATUS_*                                                               */
int epipf_run(epipf_ctx* ctx, int n_chains, const double* theta, int d, int obs_model, const double* probs,
              const uint64_t* keys, const uint32_t* filter_index, const int32_t* active, int resample_mode,
              double* log_zetas_out, int32_t* status_out);

/* epipf_run, then the path sampler of epipf_path_sample on the same stream before the results come back: one round
 * trip per MH iteration instead of two (pmcmc.py:360-362 -- particle_filter, then particle_path_sampler).
 *   chosen [n_chains]: the final particle of each chain's sampled path (the host's np.random.randint(0, N) draw,
 *                      taken before the filter -- epipf.pmcmc peeks it off the RandomState without consuming it),
 *                      or -1 for none
 *   traj_out [n_chains*T*C] int32: the sampled trajectories; zeros for chains with chosen -1 or a status other than
 *                      EPIPF_STATUS_OK (the reference draws no path after a degenerate filter) */
int epipf_run_sampled(epipf_ctx* ctx, int n_chains, const double* theta, int d, int obs_model, const double* probs,
                      const uint64_t* keys, const uint32_t* filter_index, const int32_t* active, int resample_mode,
                      const int32_t* chosen, double* log_zetas_out, int32_t* status_out, int32_t* traj_out);

/* Copy the last run's history: hidden [n_chains*T*N*C] int32 (compartment counts), ancestry [n_chains*T*N]
 * int32 (row 0 zeros, as pmcmc.py:152).  Either pointer may be NULL. */
int epipf_copy_history(epipf_ctx* ctx, int n_chains, int32_t* hidden_out, int32_t* ancestry_out);

/* On-device particle_path_sampler (pmcmc.py:236-248, including its ancestry[p] indexing) for each chain of
 * the last run; chosen [n_chains] is the host's np.random.randint(0, N) draw.  traj_out [n_chains*T*C].
 * A chain whose last run was not EPIPF_STATUS_OK (degenerate or skipped) gets zeros: its history is not walked. */
int epipf_path_sample(epipf_ctx* ctx, int n_chains, const int32_t* chosen, int32_t* traj_out);

/* Batched last-value SSA from n states [n*C] over [0, max_time] (gillespie_algo.py *_simulate with
 * last_values_only=True).  State j draws SSA event k from counter (k, j, step, filter_index). */
int epipf_simulate(epipf_ctx* ctx, int n, const int32_t* states_in, const double* theta, int d,
                   double max_time, uint64_t key, uint32_t filter_index, uint32_t step, int32_t* states_out,
                   int64_t* events_out);

/* Batched full-path SSA (gillespie_algo.py *_simulate with last_values_only=False, :68-75 / :139-146 /
 * :218-233): the same draws and final states as epipf_simulate, plus every event's time and the state after it.
 * Trajectory j keeps its first max_events events: times_out [n*max_events] (row j: its event times, ascending),
 * states_out [n*max_events*C]; n_events_out [n] is its full event count (> max_events: the rows hold the first
 * max_events only, call again with a larger buffer); final_out [n*C] (or NULL) its last state.  The event times
 * are the reference's clock bit for bit.  The initial state (time 0.0) is the caller's input. */
int epipf_simulate_path(epipf_ctx* ctx, int n, const int32_t* states_in, const double* theta, int d,
                        double max_time, uint64_t key, uint32_t filter_index, uint32_t step, int max_events,
                        double* times_out, int32_t* states_out, int32_t* n_events_out, int32_t* final_out);

/* Posterior-predictive forecast: n_draws posterior draws, each with its own parameters theta[i] ([n_draws*d]) and its
 * own start state states[i] ([n_draws*C]), `replicates` trajectories per draw, all in one launch.  Each trajectory is
 * the continuous path of epipf_simulate_path over [0, horizon] binned on the device to one row per day: row j
 * (0..horizon-1) is the state after the last event with time < j + 1, and a day without an event repeats the previous
 * row (tests/pred_tmps.py:58-63: the last index with floor(time) == j, else the previous row).
 * Draw i, replicate r draws SSA event k from counter (k, r, step, filter_index + i) (uint32 wrap): its forecast is
 * epipf_simulate_path of `replicates` copies of states[i] with theta[i] at filter index filter_index + i, bit for bit,
 * whatever else is in the batch.
 *   rows_out [n_draws*replicates*horizon*C] int32, or NULL (nothing per trajectory leaves the device)
 *   sums_out [horizon*C]: sum of every row cell over the n_draws*replicates trajectories (exact)
 *   hist_out [horizon*C*bins] uint32, or NULL: hist[j][c][v] = trajectories whose row j has value v in compartment c;
 *            bins must exceed the largest start-state total (every model conserves it)
 *   events_out (or NULL): accepted events of the whole batch
 * horizon >= 1, replicates >= 1, n_draws*replicates <= INT32_MAX (< 2^30, and horizon*C <= 65535*64, with rows_out);
 * n_draws == 0 returns EPIPF_OK with zeros. */
int epipf_forecast(epipf_ctx* ctx, int n_draws, int replicates, int horizon, const double* theta, int d,
                   const int32_t* states, uint64_t key, uint32_t filter_index, uint32_t step, int32_t* rows_out,
                   int64_t* sums_out, uint32_t* hist_out, int bins, int64_t* events_out);

/* Forecast summaries: functionals of the whole continuous path of every trajectory of epipf_forecast.
 * A call with the same arguments describes the same paths as epipf_forecast, bit for bit (draw i, replicate r, event k:
 * counter (k, r, step, filter_index + i)), and a draw depends on nothing else in its batch.  With i(t) the infectious
 * count after the events up to time t (SIR and SEIR: I; the subgroup models: the sum of I_g), per trajectory:
 *   peak             the maximum of i over the start state and every accepted event
 *   peak_time        the time of the first accepted event after which i == peak (the clock value epipf_simulate_path
 *                    reports for it); 0.0 when no event exceeds the start value
 *   extinction_time  the time of the accepted event after which nobody is infectious (SEIR: nor exposed); 0.0 when the
 *                    start state is already so; +inf when the path is still active at the horizon
 *   infections       susceptibles (summed over groups) at the start minus those of the final state
 *   events           accepted events
 * peak_out, peak_time_out, extinction_time_out, infections_out, events_out: [n_draws*replicates] each, draw-major, or
 * all five NULL (nothing per trajectory leaves the device).  Reductions over the trajectories, exact integers:
 *   totals_out [4]: sum of peak, sum of infections, extinct trajectories, sum of events
 *   peak_hist_out, infections_hist_out [bins] uint32, or both NULL: trajectories with each value; bins must exceed the
 *            largest start-state total
 *   peak_day_out [horizon] uint32: trajectories with min(floor(peak_time), horizon - 1) equal to each day
 *   extinct_day_out [horizon+1] uint32: extinct trajectories by min(floor(extinction_time), horizon - 1); entry
 *            [horizon] counts those that are not extinct.  The running sum up to day k is the number of trajectories
 *            whose epipf_forecast row k has nobody infected, except that an extinction event at exactly
 *            t = horizon, which no row holds, counts in entry [horizon - 1]
 *   extinct_per_draw_out [n_draws] uint32, or NULL: extinct trajectories of each draw
 * Limits as epipf_forecast's; n_draws == 0 returns EPIPF_OK with zeros. */
int epipf_forecast_summary(epipf_ctx* ctx, int n_draws, int replicates, int horizon, const double* theta, int d,
                           const int32_t* states, uint64_t key, uint32_t filter_index, uint32_t step,
                           int32_t* peak_out, double* peak_time_out, double* extinction_time_out,
                           int32_t* infections_out, int32_t* events_out, int64_t* totals_out,
                           uint32_t* peak_hist_out, uint32_t* infections_hist_out, int bins, uint32_t* peak_day_out,
                           uint32_t* extinct_day_out, uint32_t* extinct_per_draw_out);

/* Particle smoother: daily state estimates over the observed window from a filter's whole history
 * h[T][N][C] (hidden), a[T][N] (ancestry), as a backward pass of integer multiplicities.  With shift = `lineage`:
 *   m[T-1][i] = 1;  m[p][i] = sum of m[p+1][j] over the j with a[p+shift][j] == i  (p = T-2 .. 0)
 *   sums[p][c] = sum_i m[p][i] h[p][i][c]  (exact);  lineages[p] = #{i : m[p][i] > 0}
 *   quantile q of cell (p, c) = the smallest v with sum of m[p][i] over h[p][i][c] <= v  >=  max(ceil(q N), 1)
 *                               (np.quantile(..., method="inverted_cdf") over the N lineages; `bins` when values >= bins,
 *                               which are not counted, keep the counts below the rank)
 * EPIPF_LINEAGE_REFERENCE follows a[p] as particle_path_sampler does (pmcmc.py:236-248): every output is the statistic
 * over the N trajectories that sampler returns for chosen = 0..N-1.  EPIPF_LINEAGE_GENEALOGY follows a[p+1], the parent
 * of a day-(p+1) particle: the true ancestral tree.  EPIPF_SMOOTH_PREDICTIVE sets m = 1 on every day (the particle cloud
 * itself; lineages = N).  The mean is sums / N.
 *   q [n_q] in [0, 1]; n_q == 0: no histogram is built (quant_out may be NULL, bins is ignored)
 *   sums_out [n*T*C]; quant_out [n*n_q*T*C]; lineages_out [n*T]
 * epipf_smooth: the first n_chains chains of the last run (EPIPF_ESTATE before any); a chain whose last status was not
 * EPIPF_STATUS_OK gets zeros and its history is not walked.  epipf_smooth_history: the same kernels on host arrays
 * hidden [n*T*N*C] (>= 0) and ancestry [n*T*N] (in [0, N)); any context works, its model and N are ignored.
 * The histograms (T*C*bins*4 bytes per chain, at most 256 MiB) stay on the device; chains are processed in slices when
 * together they exceed the call's scratch budget.  T == 1 is valid; C <= 64. */
#define EPIPF_LINEAGE_REFERENCE 0
#define EPIPF_LINEAGE_GENEALOGY 1
#define EPIPF_SMOOTH_SMOOTHING 0
#define EPIPF_SMOOTH_PREDICTIVE 1
int epipf_smooth(epipf_ctx* ctx, int n_chains, int lineage, int kind, const double* q, int n_q, int bins,
                 int64_t* sums_out, int32_t* quant_out, int32_t* lineages_out);
int epipf_smooth_history(epipf_ctx* ctx, int n, int T, int N, int C, const int32_t* hidden, const int32_t* ancestry,
                         int lineage, int kind, const double* q, int n_q, int bins, int64_t* sums_out,
                         int32_t* quant_out, int32_t* lineages_out);

/* Fixed-lag smoother (Kitagawa 1996): day p estimated from the particles of day
 * e(p) = min(p + lag, T-1) traced back to day p, with the same history, `lineage`, outputs and quantile rule as above:
 *   w[e(p)][i] = 1;  w[q][i] = sum of w[q+1][j] over the j with a[q+shift][j] == i  (q = e(p)-1 .. p);  m[p] = w[p]
 *   sums[p][c] = sum_i m[p][i] h[p][i][c];  lineages[p] = #{i : m[p][i] > 0};  sum_i m[p][i] = N on every day
 * lag == 0 is EPIPF_SMOOTH_PREDICTIVE and lag >= T-1 is EPIPF_SMOOTH_SMOOTHING, bit for bit; lag == 1 with
 * EPIPF_LINEAGE_GENEALOGY is the filtering distribution (the resampled parents); lineages[p] does not increase with
 * lag.  lag < 0 is EPIPF_EINVAL; every other rule (state, n, q, bins, C <= 64, the histogram cap, the contents of
 * hidden and ancestry, chains that did not run, slicing under the scratch budget) is epipf_smooth's and
 * epipf_smooth_history's.  Each (chain, day) is one workgroup's window, so one chain occupies up to T compute units. */
int epipf_smooth_lag(epipf_ctx* ctx, int n_chains, int lineage, int lag, const double* q, int n_q, int bins,
                     int64_t* sums_out, int32_t* quant_out, int32_t* lineages_out);
int epipf_smooth_lag_history(epipf_ctx* ctx, int n, int T, int N, int C, const int32_t* hidden, const int32_t* ancestry,
                             int lineage, int lag, const double* q, int n_q, int bins, int64_t* sums_out,
                             int32_t* quant_out, int32_t* lineages_out);

/* Standalone resampler: out[j] = numpy legacy choice(range(n), n, p=w/sum(w)) given uniforms u[j].
 * Returns EPIPF_STATUS_DEGENERATE (as a positive value) where numpy raises ValueError. */
int epipf_resample(epipf_ctx* ctx, int n, const double* w, const double* u, int32_t* out,
                   int64_t* fallbacks_out);

/* ABC rejection sampling, abc_algo.py:17-109, for the SIR model (any context works; its model is ignored).
 *   Y [T*3]: observed_data (S, I, R per day); initial counts ~ Poisson(Y[0].astype(int)), abc_algo.py:38-39
 *   priors [4]: beta lo, hi, gamma lo, hi (uniform priors, abc_algo.py:35-36)
 * Trial t of run `run_index` draws from the keyed ABC stream: prior (0, t, 3<<24, run),
 * initial count c (c, t, 4<<24, run), SSA event k (k, t, 5<<24, run).  t < 2^32.
 *
 * epipf_abc: the first no_of_samples trials with distance <= threshold, in trial order (the reference's
 * sequential while loop).  theta_out [no_of_samples*2] (beta, gamma); traj_out [no_of_samples*T*4] rows
 * (day, S, I, R) exactly as abc_algo returns them.  At most max_trials trials are run (the reference loops
 * forever when the threshold is unreachable): *accepted_out < no_of_samples then.  *trials_out = the trial
 * count the reference reports (index of the last accepted trial + 1; max_trials when short).
 * batch <= 0 picks batch sizes automatically (growing from 16k trials to 1M).                              */
int epipf_abc(epipf_ctx* ctx, const double* Y, int T, int no_of_samples, double threshold, const double* priors,
              uint64_t key, uint32_t run_index, int64_t max_trials, int batch, double* theta_out, double* traj_out,
              int64_t* trials_out, int32_t* accepted_out);

/* Trials [t0, t0+n): theta_out [n*2]; rows_out [n*T*3] int32 (S, I, R per day) or NULL; dist_out [n] or NULL. */
int epipf_abc_trials(epipf_ctx* ctx, const double* Y, int T, const double* priors, uint64_t key, uint32_t run_index,
                     uint32_t t0, int n, double* theta_out, int32_t* rows_out, double* dist_out, int64_t* events_out);

/* ABC-SMC (population Monte Carlo ABC with a uniform perturbation kernel) for the SIR model: the
 * sequential layer over the rejection sampler.  One run keeps one global trial counter t across its generations
 * (t0 = the trials the earlier generations used); trial t takes its initial counts and SSA events from the counters
 * above whatever its generation, and its proposal from the domain 6<<24: block (0, t, 6<<24, run) selects the
 * ancestor, block (1, t, 6<<24, run) perturbs beta (words 0, 1) and gamma (words 2, 3).
 *
 * epipf_abc_smc_generation: one generation.  n_prev == 0 is the prior stage: epipf_abc from trial t0 (the same theta,
 * trajectories and trial count; ancestors -1; prev_* and half_width unused).  n_prev > 0: trial t draws the ancestor
 * j = min(searchsorted(prev_cdf, u_sel, 'right'), n_prev - 1) (prev_cdf [n_prev]: the previous weights' normalised
 * cumulative sum, non-decreasing and ending at exactly 1), proposes theta*_c = prev_theta[j][c] + half_width[c] *
 * (2 u_c - 1), is rejected without simulation (distance +inf) when theta* leaves the prior box lo_c <= theta*_c <=
 * hi_c, and otherwise runs as an ABC trial with theta = theta*.  The first no_of_samples trials with
 * distance <= threshold are accepted in trial order: theta_out [n*2], traj_out [n*T*4], dist_out [n] their distances,
 * ancestor_out [n] their ancestors.  t0 + max_trials <= 2^32; *trials_out counts from t0 by epipf_abc's rule (index
 * of the last accepted trial - t0 + 1; max_trials when short); batch as epipf_abc.
 *
 * epipf_abc_smc_weights: den_out[i] = sum over j, in j order, of prev_w[j] where |theta[i][c] - prev_theta[j][c]| <=
 * half_width[c] for both c (else +0.0): the denominator of sample i's weight under a uniform prior and kernel,
 * bit-equal to np.cumsum(np.where(mask, prev_w, 0.0))[-1].  theta [n*2], prev_theta [n_prev*2], prev_w [n_prev]. */
int epipf_abc_smc_generation(epipf_ctx* ctx, const double* Y, int T, int no_of_samples, double threshold,
                             const double* priors, const double* prev_theta, const double* prev_cdf, int n_prev,
                             const double* half_width, uint64_t key, uint32_t run_index, uint32_t t0,
                             int64_t max_trials, int batch, double* theta_out, double* traj_out, double* dist_out,
                             int32_t* ancestor_out, int64_t* trials_out, int32_t* accepted_out);
int epipf_abc_smc_weights(epipf_ctx* ctx, const double* theta, int n, const double* prev_theta, const double* prev_w,
                          int n_prev, const double* half_width, double* den_out);

/* Iterated filtering (IF2: Ionides, Nguyen, Atchade, Stoev, King, PNAS 2015) for the SIR (d = 2) and SEIR
 * (d = 3) models: a maximum-likelihood search.  n_searches independent searches run as the chains of one batch; each
 * carries a swarm of n_particles parameter vectors, one per particle.  Iteration m = 0..iterations-1 of search s is one
 * pass of epipf_run's filter at filter index filter_index0[s] + m (uint32 wrap) -- the same initial states, weights,
 * log_zeta, multinomial resampling draws and SSA counters -- in which particle j's parameters are jittered at every step p:
 *   theta_0[j] = perturb(swarm[j], j, 0);  theta_p[j] = perturb(theta_{p-1}[ancestor of j], j, p), p = 1..T-1
 *   perturb(theta, j, p)[c] = |theta[c] + half_widths[m][c] * (2 u - 1)| (reflection at 0), u = U(words 2(c%2), 2(c%2)+1)
 *                             of the Philox block (c / 2, j, (p & 0xFFFFFF) | 7 << 24, f)
 * and particle j's day p runs with the rates theta_p[j].  After the pass the swarm is theta_{T-1}.
 *   swarm_inout [n_searches*N*d]: the start swarms (every entry finite and >= 0), replaced by the final ones
 *   half_widths [iterations*d] (finite, >= 0);  probs [n_searches]: fixed, as epipf_run's
 *   log_zetas_out [n_searches*iterations*T] or NULL: each pass's log_zeta (the likelihood of the perturbed model)
 *   mean_out [n_searches*iterations*d]: the swarm's component means after each iteration
 *   iterations_done_out [n_searches]: completed iterations;  status_out [n_searches]: EPIPF_STATUS_*
 * A step whose weights sum to 0 or NaN ends its search (EPIPF_STATUS_DEGENERATE): its swarm comes back as the failed
 * iteration found it, its mean_out / log_zetas_out rows from that iteration on are NaN, and the other searches are not
 * affected.  T == 1 is valid (only the step-0 jitter runs).  Every launch of the call is enqueued without host
 * synchronisation.  Afterwards epipf_copy_history / epipf_path_sample / epipf_smooth see the last executed pass of each
 * search.  EPIPF_EINVAL on a subgroup context: epipf_iterated_filtering_subgroups runs those models.
 * epipf_get_stats afterwards: resample_fallbacks of this call, and at EPIPF_PROFILE_COUNTERS its events,
 * lane_iterations, wave_lane_slots, ssa_exact_lanes and ssa_exact_waves (a failed iteration's steps before the dying one
 * included).  The device counters are left cleared: the next epipf_run reports its own counts only. */
int epipf_if2(epipf_ctx* ctx, int n_searches, int iterations, double* swarm_inout, int d, const double* half_widths,
              int obs_model, const double* probs, const uint64_t* keys, const uint32_t* filter_index0,
              double* log_zetas_out, double* mean_out, int32_t* iterations_done_out, int32_t* status_out);

/* epipf_if2 for the subgroup models (EPIPF_SIR_SUBGROUPS, EPIPF_SIR_SUBGROUPS2) with 2 <= G <= 4 groups (DESIGN.md
 * §17.1).  The definition above holds word for word with d = G*G + 1 and theta laid out as beta[G][G] row-major, then
 * gamma (epipf_run's layout): component c draws from block c / 2, so d = 5 and d = 17 use the first half of their last
 * block only.  A half-width of 0 leaves a component bit-identical, which fixes entries of the contact matrix (for
 * example off-diagonals at 0).  EPIPF_SIR_SUBGROUPS2 weighs the sums over the groups, as its filter does.  Arguments,
 * returns, status, statistics and what the history calls see afterwards are epipf_if2's.  EPIPF_EINVAL on a SIR or SEIR
 * context (epipf_if2 runs those) and on G = 1 or G > 4: the wider models read their rates by wave-uniform address,
 * which a per-particle theta is not. */
int epipf_iterated_filtering_subgroups(epipf_ctx* ctx, int n_searches, int iterations, double* swarm_inout, int d,
                                       const double* half_widths, int obs_model, const double* probs,
                                       const uint64_t* keys, const uint32_t* filter_index0, double* log_zetas_out,
                                       double* mean_out, int32_t* iterations_done_out, int32_t* status_out);

/* Time-varying rates for the SIR (d = 2) and SEIR (d = 3) models.
 * epipf_walk_filter is one pass of epipf_if2 (iterations = 1, m = 0: the same perturb, Philox domain 7 << 24, counters,
 * weights, resampling, SSA and degeneracy rule) with a half-width vector per chain, half_widths [n_chains*d] (finite,
 * >= 0; an entry of 0 keeps that component bit for bit), in which every day's parameters theta_p are kept on the device
 * (theta_hist f64 [chain][T][d][N], allocated on first use, regrown when a call needs more, freed by epipf_destroy;
 * EPIPF_ENOMEM names the bytes asked for).  It is the bootstrap filter of the model "theta follows a reflected uniform
 * random walk": log_zetas_out[s][T-1] estimates that model's likelihood at chain s's step widths.
 *   swarm_in [n_chains*N*d] (finite, >= 0): the sample theta_0 is jittered from;  probs, keys, filter_index [n_chains]
 *   log_zetas_out [n_chains*T];  status_out [n_chains]
 * hidden, ancestry, status and log_zeta are the context's: epipf_copy_history, epipf_path_sample and epipf_smooth see the
 * pass afterwards.  A chain that degenerates at step p keeps its rows < p; its log_zetas from p on are -inf.
 * EPIPF_EINVAL on a subgroup context. */
int epipf_walk_filter(epipf_ctx* ctx, int n_chains, const double* swarm_in, int d, const double* half_widths,
                      int obs_model, const double* probs, const uint64_t* keys, const uint32_t* filter_index,
                      double* log_zetas_out, int32_t* status_out);

/* theta_out [n_chains*T*N*d]: the parameter history of the last epipf_walk_filter (NaN in a degenerate chain's rows from
 * its dying step on).  EPIPF_ESTATE before any epipf_walk_filter, and after another run (epipf_run, epipf_if2, ...) has
 * overwritten the context's history. */
int epipf_walk_history(epipf_ctx* ctx, int n_chains, double* theta_out);

/* The smoothed parameters.  Particle i of day p has V = d + 1 quantities: v_c = theta_p[i][c] + 0.0 for c < d, and
 *   v_d = R = (theta_p[i][0] * (double)S_p[i]) / (theta_p[i][d-1] * P) + 0.0, +inf where the denominator is 0.0
 * (S = compartment 0, P = the population total; no contraction).  With m[p][i] the multiplicities of epipf_smooth_lag at
 * `lag` (lag < 0 or lag >= T-1: the full smoother; lag 0: the particle cloud) under `lineage`:
 *   lineages_out [n*T]        #{i : m[p][i] > 0}
 *   mean_out [n*T*V]          sum_i m[p][i] v_k[i] / N over the i with m > 0, summed in a fixed order (no floating-point
 *                             atomics: the same bits on every run; within (N + 1) 2^-53 relative of the exact value)
 *   quant_out [n*n_q*T*V]     the smallest v_k[i] whose cumulative multiplicity reaches max(ceil(q N), 1): numpy's
 *                             inverted_cdf quantile of the values repeated m times, an element of the input, bit for bit
 *                             (NULL with n_q = 0)
 * Chains whose status is not EPIPF_STATUS_OK are not walked: their rows are zeros.  EPIPF_ESTATE as epipf_walk_history. */
int epipf_walk_smooth(epipf_ctx* ctx, int n_chains, int lineage, int lag, const double* q, int n_q, double* mean_out,
                      double* quant_out, int32_t* lineages_out);

/* The same reduction on host arrays hidden [n*T*N*C] (only compartment 0 is read), ancestry [n*T*N] and theta
 * [n*T*N*d], 1 <= d <= 3, with P = population_total (finite, > 0); the context's own shape is ignored, as in
 * epipf_smooth_history.  EPIPF_EINVAL, naming the first offending index, for a negative, NaN or infinite theta entry, a
 * negative hidden entry or an ancestor outside [0, N). */
int epipf_walk_smooth_history(epipf_ctx* ctx, int n, int T, int N, int C, int d, const int32_t* hidden,
                              const int32_t* ancestry, const double* theta, double population_total, int lineage,
                              int lag, const double* q, int n_q, double* mean_out, double* quant_out,
                              int32_t* lineages_out);

/* Incidence observations for the SIR and SEIR models: the filter weighted by reported transition counts
 * instead of the compartments.  counts [D*F], one row per day d = 1..D for the interval (d-1, d], F = 2 columns for SIR
 * (infections S' - S, removals R - R') and 3 for SEIR (exposures S' - S, onsets (I + R) - (I' + R'), removals R - R'),
 * x' the particle's parent state and x its new one; NaN = not reported.  The pass has T = D + 2 rows: row 0 the initial
 * draw (weight 1), rows 1..D the days, row D + 1 one more resampling on day D's weights and one more propagation, so
 * log_zetas_out[s][D+1] is the log-likelihood of every report, log_zetas_out[s][1] is exactly 0, and the trajectories
 * and the smoother see the last report.  With rep[p][k] = "counts row p column k is reported",
 *   acc_p[j][k] = flow_p[j][k] + (cumulate && !rep[p-1][k] ? acc_{p-1}[a_p[j]][k] : 0),   acc_0 = 0
 *   w_p[j]      = product over the k with rep[p][k], in column order from 1.0, of
 *                 EPIPF_OBS_BINOMIAL: the binomial pmf of counts[p][k] out of acc_p[j][k] at probs[s]
 *                 EPIPF_OBS_NORMAL:   the normal pdf of counts[p][k] at mean acc_p[j][k], sd probs[s] acc_p[j][k] + 1e-4
 * (a row with nothing reported weighs 1).  cumulate = 0: a report counts its day alone; 1: everything since that
 * column's previous report (ping-pong accumulator int32 [2][n_chains][F][N] on the device, allocated on first use,
 * regrown when a call needs more, freed by epipf_destroy; EPIPF_ENOMEM names the bytes asked for, also when they exceed
 * the budget EPIPF_INCIDENCE_ACC_BYTES of the environment at epipf_create).  Resampling is multinomial; Philox domains,
 * counters, the SSA and the degeneracy rule are epipf_run's, and so are theta, keys, filter_index and active.
 *   log_zetas_out [n_chains*(D+2)];  status_out [n_chains]
 * The reports live in a device buffer of their own: the observations of epipf_set_observations are untouched (and not
 * needed; epipf_set_population is).  The context's run length becomes D + 2: epipf_copy_history, epipf_path_sample,
 * epipf_smooth and epipf_smooth_lag see the pass afterwards; epipf_walk_history is EPIPF_ESTATE after it.
 * EPIPF_EINVAL, naming the first offending index: a subgroup context; D < 1 or D + 2 > t_max; a report that is infinite
 * or negative, or (binomial) not an integer; an active chain's theta entry negative, NaN or infinite; an active chain's
 * probs NaN, infinite, negative or (binomial) above 1. */
int epipf_run_incidence(epipf_ctx* ctx, int n_chains, const double* theta, int d, int obs_model, const double* probs,
                        const uint64_t* keys, const uint32_t* filter_index, const int32_t* active, const double* counts,
                        int D, int cumulate, double* log_zetas_out, int32_t* status_out);

/* R_t from case counts for the SIR and SEIR models: the random-walk filter of epipf_walk_filter weighted
 * by the reports of epipf_run_incidence.  Every particle carries its own theta, jittered at every step by the
 * half-widths of its chain (the same perturb, Philox domain 7 << 24; no new domain, counter layout or stream), over the
 * T = D + 2 rows of the incidence pass, with its flows, accumulator and product weight as defined above.
 *   swarm_in [n_chains*N*d], half_widths [n_chains*d]: epipf_walk_filter's rules;  probs, keys, filter_index [n_chains]
 *   counts [D*F], D, cumulate, probs: epipf_run_incidence's rules and error texts (every chain runs: no `active`)
 *   log_zetas_out [n_chains*(D+2)];  status_out [n_chains]
 * theta_hist is kept over the D + 2 rows and the run length becomes D + 2: epipf_walk_history, epipf_walk_smooth,
 * epipf_copy_history, epipf_path_sample, epipf_smooth, epipf_smooth_lag and epipf_incidence_smooth see the pass
 * afterwards.  A chain that degenerates at step p has log_zetas -inf from row p on and NaN theta rows from p on.
 * EPIPF_EINVAL on a subgroup context; EPIPF_ESTATE without epipf_set_population (observations are not needed);
 * EPIPF_ENOMEM as epipf_walk_filter (theta_hist) and epipf_run_incidence (the accumulator and its budget). */
int epipf_incidence_walk(epipf_ctx* ctx, int n_chains, const double* swarm_in, int d, const double* half_widths,
                         int obs_model, const double* probs, const uint64_t* keys, const uint32_t* filter_index,
                         const double* counts, int D, int cumulate, double* log_zetas_out, int32_t* status_out);

/* The smoothed true flows of the last epipf_run_incidence or epipf_incidence_walk (EPIPF_ESTATE before one, and after
 * any other run has overwritten the context's history).  With T = D + 2 and F the model's flow columns,
 *   flow[p][i][k] = the flows of epipf_run_incidence between hidden[p-1][ancestry[p][i]] and hidden[p][i] for p >= 1,
 *                   0 in row 0: the day's own flow, also under cumulate
 * formed on the device and reduced as epipf_smooth_lag reduces a history of F compartments, under the multiplicities of
 * EPIPF_LINEAGE_GENEALOGY (the flows are defined by the true parent) at `lag` (lag < 0 or lag >= T-1: the full
 * smoother; 0: the particle cloud):
 *   sums_out [n*T*F];  quant_out [n*n_q*T*F] (NULL with n_q = 0);  lineages_out [n*T]
 * The quantile rule, bins (a flow is at most the population total), slicing and the zeros of chains that are not
 * EPIPF_STATUS_OK are epipf_smooth_lag's. */
int epipf_incidence_smooth(epipf_ctx* ctx, int n_chains, int lag, const double* q, int n_q, int bins, int64_t* sums_out,
                           int32_t* quant_out, int32_t* lineages_out);

/* Negative-binomial reporting for the incidence filters: overdispersed case counts.  A report y of a
 * column whose accumulated flow is n (acc_p[j][k] above) weighs, with rho = probs[s] (a mean ratio: it may exceed 1) and
 * kappa = dispersion[s],
 *   m = rho n;   m > 0 false: (y == 0 ? 1 : 0), a point mass at 0;   else, with t = kappa + m,
 *   exp((c + kappa (log kappa - log t)) + y (log m - log t)),   c = lgamma(y + kappa) - lgamma(kappa) - lgamma(y + 1)
 * in this order in plain doubles, log glibc's, c formed on the host in binary128 and rounded once (epipf_negbin_coefficients):
 * the negative-binomial pmf of mean m and variance m + m^2 / kappa.  Everything else -- rows, the product over the
 * reported columns, cumulate, degeneracy, resampling, Philox domains, the SSA, and the context's state afterwards -- is
 * epipf_run_incidence's and epipf_incidence_walk's, whose arguments these take without obs_model and with
 * dispersion [n_chains]; their validation and error texts hold, with these differences: a report must be an integer;
 * an active chain's probs must be finite and >= 0 (and, being handed to a log that is defined for normal doubles, 0 or
 * in [2^-1022, 2^990]); its dispersion must lie in [2^-1022, 1e6] -- the factor's rounding error is about
 * kappa (|log kappa| + |log t|) 2^-53, 3e-9 at 1e6, and the Poisson limit beyond is out of scope.  The constants live in
 * two device buffers of doubles, [n_chains][D+2][F] and [n_chains][2], allocated on first use, regrown on demand and
 * freed by epipf_destroy. */
int epipf_run_incidence_negbin(epipf_ctx* ctx, int n_chains, const double* theta, int d, const double* probs,
                               const double* dispersion, const uint64_t* keys, const uint32_t* filter_index,
                               const int32_t* active, const double* counts, int D, int cumulate, double* log_zetas_out,
                               int32_t* status_out);
int epipf_incidence_walk_negbin(epipf_ctx* ctx, int n_chains, const double* swarm_in, int d, const double* half_widths,
                                const double* probs, const double* dispersion, const uint64_t* keys,
                                const uint32_t* filter_index, const double* counts, int D, int cumulate,
                                double* log_zetas_out, int32_t* status_out);

/* out[i] = c(y[i], dispersion) as above (exactly 0 at y = 0): the constants the two entry points hand to the device.
 * Host only; no GPU involved.  EPIPF_EINVAL for a y that is negative, infinite, NaN or not an integer, and for a
 * dispersion outside (0, 1e6]. */
int epipf_negbin_coefficients(const double* y, int n, double dispersion, double* out);

/* The device's restatement of glibc's log (the reference's math.log / numpy legacy exponential),
 * evaluated on the host CPU with the same code and table: out[i] = log(x[i]) bit for bit for normal x[i] > 0.
 * For tests of that restatement; no GPU involved. */
int epipf_glibc_log(int64_t n, const double* x, double* out);

/* The lane-group filter's certified-clock log (clock_log_impl, csrc/epipf_device.hpp: glibc's table path without its
 * close-to-1 branch), on the host CPU with the same code and table: out[i] ~ log(x[i]) within the bound its clock
 * certificate assumes (tests/test_glibc_log.py measures it).  For tests; no GPU involved. */
int epipf_clock_log(int64_t n, const double* x, double* out);

/* Profiling levels: OFF; TIMING = HIP events around the init / step kernels (step_ms, init_ms), no effect on
 * the kernels; COUNTERS = TIMING + device counters of SSA events and lane use (a few atomics per wave). */
#define EPIPF_PROFILE_OFF 0
#define EPIPF_PROFILE_TIMING 1
#define EPIPF_PROFILE_COUNTERS 2
int epipf_set_profiling(epipf_ctx* ctx, int level);

/* Chain groups of one epipf_run on concurrent HIP streams (1..8, default 4 or EPIPF_STREAMS): each group's T-1
   step kernels run back to back on its own stream so that one group's launch tail overlaps the others' work.
   Engine tuning only, no reference counterpart; results do not depend on it.  A host that runs several contexts
   from separate threads (MH iterations pipelined with the device, epipf.pmcmc.run_pipelined) sets 1 each. */
int epipf_set_streams(epipf_ctx* ctx, int n_streams);
/* Lanes per particle in the step kernel's SSA: 0 = automatic (default; EPIPF_LANES overrides), 1 = one lane per
   particle (throughput: batches that fill the chip), 2/4/8/16 = a group of lanes draws consecutive events' Philox
   blocks in parallel and runs only the sequential decisions event by event (latency: a single chain or a few chains,
   DESIGN.md §12).  events_per_lane: events each lane of a group draws per chunk (0 = automatic).  Engine tuning only,
   no reference counterpart; results are identical for every value.  lanes > 1 on a context with G > 4 is EPIPF_EINVAL
   (lane groups exist for G <= 4), as is EPIPF_LANES > 1 at its creation. */
int epipf_set_lanes(epipf_ctx* ctx, int lanes, int events_per_lane);
int epipf_get_stats(epipf_ctx* ctx, epipf_stats* out);
int epipf_reset_stats(epipf_ctx* ctx);

/* Host side of a many-chain MH iteration (epipf.pmcmc.ChainSampler, pmcmc.py:325-406 per chain), in C: each chain's
 * numpy legacy RandomState draws made on its MT19937 state in place (mt_states[c]: the bit generator's
 * ctypes.state_address, numpy's mt19937_state), bit-identical to numpy's own and in the reference's order.  No device
 * work; status codes as the rest of the ABI.
 * epipf_mh_propose: props_out[c] = multivariate_normal(means[c], .) of pmcmc.py:330 = standard_normal(d) (even d, empty
 *   gaussian cache) times factors[c] ([d][d], mvn_factor) by dgemv (numpy's own cblas_dgemv, a function pointer:
 *   the product numpy computes for np.dot) plus means[c].
 * epipf_mh_decide: for the n chains listed in chains[] (their filters succeeded), in order: chosen_out[c] =
 *   randint(0, n_particles) (the path sampler's pick, pmcmc.py:241), then accept_out[c] = random_sample() <
 *   min(1, exp(min(lz_new[c] - lz_old[c], 0))) (the log-space acceptance, 0 for NaN). */
int epipf_mh_propose(int n_chains, int d, void* const* mt_states, const double* factors, const double* means,
                     double* props_out, void* dgemv);
int epipf_mh_decide(int n, const int32_t* chains, void* const* mt_states, int n_particles, const double* lz_new,
                    const double* lz_old, int32_t* chosen_out, int32_t* accept_out);
/* epipf_mh_peek: chosen_out[c] = the randint(0, n_particles) the next epipf_mh_decide draws for each listed chain,
 * read on a copy of its state (nothing consumed): the path sampler's picks for epipf_run_sampled, before the filter. */
int epipf_mh_peek(int n, const int32_t* chains, void* const* mt_states, int n_particles, int32_t* chosen_out);

const char* epipf_last_error(void);
int epipf_abi_version(void);
/* Largest G the subgroup models accept (8). */
int epipf_max_groups(void);
/* Hash of the library's sources and build flags (16 hex digits; "...-debug" for libepipf_debug.so).  Profiles taken
 * on one build are trusted by bench.py only for the same id. */
const char* epipf_build_id(void);
int epipf_device_count(void);

#ifdef __cplusplus
}
#endif

#endif /* EPIPF_H */
