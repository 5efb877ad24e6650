/*
 * cpecan_hip.h -- C-ABI of the MI355X (gfx950) implementation of cPecan's banded pair-HMM
 * forward / backward / posterior DP over nanopore events x reference k-mers.
 *
 * Plain C: opaque handles, plain pointers and sizes, no HIP or C++ types in any signature.
 * This is the boundary the reference's C code would link against for this path; each entry point
 * names the reference interface it replaces.  All functions return CPECAN_OK (0) or a negative
 * CPECAN_E* code; cpecan_hip_last_error() gives the message of the calling thread's last failure.
 * There is no CPU fallback: without a usable GPU every compute entry point fails with
 * CPECAN_ENODEVICE.
 */
#ifndef CPECAN_HIP_H_
#define CPECAN_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define CPECAN_OK 0
#define CPECAN_ENODEVICE (-1)  /* no HIP device / runtime error at start-up          */
#define CPECAN_EINVAL (-2)     /* bad argument                                       */
#define CPECAN_EHIP (-3)       /* a HIP call failed (message in last_error)          */
#define CPECAN_EOVERFLOW (-4)  /* an output capacity was too small                   */
#define CPECAN_EBAND (-5)      /* anchors describe an invalid band (diagonal_construct throw) */
#define CPECAN_ELIMIT (-6)     /* the context's device memory limit would be passed   */

#define CPECAN_NUM_KMERS 4096
#define CPECAN_KMER_LENGTH 6
#define CPECAN_MODEL_PARAMS 5
#define CPECAN_MODEL_TABLE_LEN (1 + CPECAN_NUM_KMERS * CPECAN_MODEL_PARAMS)
#define CPECAN_PAIR_ALIGNMENT_PROB_1 10000000 /* inc/pairwiseAligner.h:26 */

typedef struct cpecan_ctx cpecan_ctx;     /* one per (host thread, GPU): device, stream, models */
typedef struct cpecan_batch cpecan_batch; /* a set of independent alignments resident in HBM    */

/* ---- start-up ------------------------------------------------------------------------------ */
int cpecan_hip_device_count(int *count);
int cpecan_hip_ctx_create(int device, cpecan_ctx **ctx);
int cpecan_hip_ctx_destroy(cpecan_ctx *ctx);
const char *cpecan_hip_last_error(void);
const char *cpecan_hip_version(void);
/* Device memory held on behalf of a context: the blocks of its model tables and of its live batches, each at the size
 * the library's allocator handed it out (a reused block is up to a quarter larger than what was asked for).  *live: now;
 * *peak: the most since the context was made or the peak was last reset (reset_peak != 0 sets it to *live after it is
 * read).  Either may be NULL.  What the allocator keeps of released blocks for reuse belongs to no context: it is bounded
 * by CPECAN_ALLOC_CACHE_GB and given back by the trim call below. */
int cpecan_hip_ctx_memory(cpecan_ctx *ctx, int64_t *live, int64_t *peak, int32_t reset_peak);
/* A limit on that figure, in bytes; 0 (the default): none.  With a limit, an allocation that would take the context's
 * live bytes past it is not made and the call fails with CPECAN_ELIMIT -- a model create call, a batch create call, the
 * growth of an output capacity at run or readback -- and last_error names the bytes asked for and the limit.  A create
 * call that fails so has released all it took: live is what it was, and the context stays usable.  A limit below what
 * the context already holds refuses every further allocation until enough is released.  A run or a readback that
 * fails so leaves the batch as it was before the call, but for buffers it will make again: once there is room (memory
 * released, the limit raised) the same call may simply be made again (a readback whose growth of the pair buffer was
 * refused runs the batch once more first, as it would have then). */
int cpecan_hip_ctx_set_memory_limit(cpecan_ctx *ctx, int64_t bytes);

/* ---- model ---------------------------------------------------------------------------------
 * Replaces the StateMachine3 the reference builds with getStrawManStateMachine3()
 * (impl/stateMachine.c:1725) and rescales per read with emissions_signal_scaleModel() (:631):
 * transitions in the order of struct _StateMachine3 (inc/stateMachine.h:179-187), emission tables
 * in the reference's own layout (EMISSION_MATCH_PROBS / EMISSION_GAP_Y_PROBS = 1+4096*5 doubles,
 * EMISSION_GAP_X_PROBS = 4096 doubles).  The tables are read once, on the host, to derive the
 * device table (log sigma etc. use the host libm, as the reference's per-cell log() does). */
typedef struct {
    double transitions[9]; /* MATCH_CONTINUE, MATCH_FROM_GAP_X, MATCH_FROM_GAP_Y, GAP_OPEN_X,
                              GAP_OPEN_Y, GAP_EXTEND_X, GAP_EXTEND_Y, GAP_SWITCH_TO_X, GAP_SWITCH_TO_Y */
    const double *match_probs; /* [CPECAN_MODEL_TABLE_LEN] */
    const double *gap_x_probs; /* [CPECAN_NUM_KMERS]       */
    const double *gap_y_probs; /* [CPECAN_MODEL_TABLE_LEN] */
} cpecan_sm3_model;

/* Derives and uploads n models (host work is spread over `threads` OS threads, <=0: all cores);
 * ids[i] receives the handle of models[i]. */
int cpecan_hip_models_create(cpecan_ctx *ctx, const cpecan_sm3_model *models, int32_t n,
                             int32_t threads, int32_t *ids);
/* The same for n reads that share one pore model and differ by their scaling parameters only -- what
 * emissions_signal_scaleModel (impl/stateMachine.c:631-651) does to a read's copy of EMISSION_MATCH_PROBS before the
 * alignment (vanillaAlign.c:624-640): level_mean * scale + shift, level_sd * var, noise_mean * scale_sd,
 * noise_lambda * var_sd, noise_sd = sqrt(noise_mean^3 / noise_lambda).  The host takes only what needs its libm
 * (pow, sqrt and the two logs per k-mer) and uploads three doubles per k-mer per read; the device assembles the rows
 * with single IEEE operations.  The resulting device tables are bit-identical to cpecan_hip_models_create() on the
 * n host-scaled tables (tests/test_scaled_models_gpu.py), at a sixth of the upload. */
typedef struct {
    double scale, shift, var, scale_sd, var_sd;
} cpecan_read_scaling;
int cpecan_hip_models_create_scaled(cpecan_ctx *ctx, const cpecan_sm3_model *base, const cpecan_read_scaling *scalings,
                                    int32_t n, int32_t threads, int32_t *ids);
/* Test aid: copies the derived device table of strawMan model `id` to out (n_doubles receives its length; out may be
 * NULL to query the length only). */
int cpecan_hip_models_download(cpecan_ctx *ctx, int32_t id, double *out, int64_t capacity, int64_t *n_doubles);
int cpecan_hip_models_clear(cpecan_ctx *ctx);
/* The M-step of Baum-Welch changes the nine transitions and the k-mer gap probabilities only
 * (continuousPairHmm_loadTransitionsAndKmerGapProbs impl/continuousHmm.c:206-232); the per-read scaled emission
 * tables stay.  Rewrites those 9 + 4096 values in every strawMan model of the context in place (gap_x_probs may be
 * NULL: transitions only), so that batches created on the context can simply be run again for the next
 * iteration -- no table derivation, no upload. */
int cpecan_hip_models_set_transitions(cpecan_ctx *ctx, const double *transitions /*[9]*/,
                                      const double *gap_x_probs /*[CPECAN_NUM_KMERS] or NULL*/);

/* The 5-state symbol machine of DNA-against-DNA alignment: stateMachine5_construct(fiveState)
 * (impl/stateMachine.c:896-965; BASELINE configs[0]).  transitions in the order of struct
 * _StateMachine5 (inc/stateMachine.h:108-124): MATCH_CONTINUE, MATCH_FROM_SHORT_GAP_X,
 * MATCH_FROM_LONG_GAP_X, GAP_SHORT_OPEN_X, GAP_SHORT_EXTEND_X, GAP_SHORT_SWITCH_TO_X, GAP_LONG_OPEN_X,
 * GAP_LONG_EXTEND_X, GAP_LONG_SWITCH_TO_X, then the same eight for Y; emissions as
 * emissions_symbol_* reads them (:155-173): match [4x4] by (x base, y base), gaps [4].
 * Ids live in their own space (used by cpecan_hip_batch_create_dna only). */
typedef struct {
    double transitions[17];
    double match_probs[16];
    double gap_x_probs[4];
    double gap_y_probs[4];
} cpecan_sm5_model;
int cpecan_hip_models5_create(cpecan_ctx *ctx, const cpecan_sm5_model *models, int32_t n, int32_t *ids);

/* The 4-state signal machine: getStateMachine4() (impl/stateMachine.c:1750-1759, stateMachine4_cellCalculate :867-897)
 * after emissions_signal_scaleModel(): match, short gap X, short gap Y, long gap X over the strawMan emissions.
 * transitions in the member order of struct _StateMachine4 (inc/stateMachine.h:134-152): MATCH_CONTINUE,
 * MATCH_FROM_SHORT_GAP_X, MATCH_FROM_LONG_GAP_X, MATCH_FROM_SHORT_GAP_Y, GAP_SHORT_OPEN_X, GAP_SHORT_EXTEND_X,
 * GAP_SHORT_OPEN_Y, GAP_SHORT_EXTEND_Y, GAP_LONG_OPEN_X, GAP_LONG_EXTEND_X, GAP_LONG_SWITCH_TO_X; tables as in the
 * strawMan model above (the machine's k-mer gap table is all zeros as getStateMachine4 leaves it). */
typedef struct {
    double transitions[11];
    const double *match_probs; /* [CPECAN_MODEL_TABLE_LEN] */
    const double *gap_x_probs; /* [CPECAN_NUM_KMERS]       */
    const double *gap_y_probs; /* [CPECAN_MODEL_TABLE_LEN] */
} cpecan_sm4_model;
int cpecan_hip_models4_create(cpecan_ctx *ctx, const cpecan_sm4_model *models, int32_t n, int32_t *ids);

/* The 3-state "vanilla" signal machine: getSignalStateMachine3Vanilla() (impl/stateMachine.c:1761) after
 * emissions_signal_scaleModel().  Fields as in struct _StateMachine3Vanilla (inc/stateMachine.h:189-205):
 * the two transition fudge factors (stateMachine3Vanilla_setStrandTransitionsToDefaults :1291), the three
 * end-state log-probabilities, the match and extra-event tables in the reference's layout and the 60
 * skip-bin values of EMISSION_GAP_X_PROBS (beta[30] | alpha[30], :284-297).  X elements are read as
 * sequence_getKmer2 does (:320-325); k-mers must be ACGT-only (the reference computes NaN otherwise).
 * Ids live in their own space (used by cpecan_hip_batch_create_vanilla only). */
typedef struct {
    double m_to_y_not_x, e_to_e;
    double end_match_prob, end_from_x_prob, end_from_y_prob;
    const double *match_probs; /* [CPECAN_MODEL_TABLE_LEN] */
    const double *skip_probs;  /* [60]                     */
    const double *gap_y_probs; /* [CPECAN_MODEL_TABLE_LEN] */
} cpecan_vanilla_model;
int cpecan_hip_modelsv_create(cpecan_ctx *ctx, const cpecan_vanilla_model *models, int32_t n,
                              int32_t threads, int32_t *ids);
/* The same for n reads of one strand: `base` holds the strand's unscaled tables, fudge factors and end values, and the
 * reads differ by their scaling parameters only.  emissions_signal_scaleModel (impl/stateMachine.c:631-651) rewrites
 * the match table alone (level_mean * scale + shift, level_sd * var, noise_mean * scale_sd, noise_lambda * var_sd; the
 * noise sd it also rewrites is not part of a vanilla row), so the host takes only what needs its libm, in the
 * reference's order of evaluation -- log(level_sd * var) and log(noise_lambda * var_sd), two doubles per k-mer and
 * read, spread over `threads` OS threads -- and the device assembles the blocks: header, extra-event half of every row
 * and the "not a k-mer" row from the base block, the match half with single IEEE operations.  The resulting device
 * blocks are bit-identical to cpecan_hip_modelsv_create on the n host-scaled tables
 * (tests/test_vanilla_scaled_models_gpu.py), at a sixth of the upload.  The vanilla table lives on the device only: both
 * entry points append to it there (a table that grows is copied device to device), ids count up across the two. */
int cpecan_hip_modelsv_create_scaled(cpecan_ctx *ctx, const cpecan_vanilla_model *base, const cpecan_read_scaling *scalings,
                                     int32_t n, int32_t threads, int32_t *ids);
/* Test aid: copies the derived device block of vanilla model `id` to out (n_doubles receives its length; out may be
 * NULL to query the length only). */
int cpecan_hip_modelsv_download(cpecan_ctx *ctx, int32_t id, double *out, int64_t capacity, int64_t *n_doubles);
/* The M-step of this machine changes the 60 skip-bin values only (vanillaHmm_loadKmerSkipBinExpectations,
 * impl/continuousHmm.c); the per-read scaled rows stay.  Rewrites, in every vanilla model of the context and in place,
 * the 30 x 5 log transition probabilities derived from them.  log a_my and log a_mm depend on the model's own
 * m_to_y_not_x, which differs between strands: the host takes the 150 logs once per distinct value with its libm, as
 * the create calls do, and every model receives the set that belongs to its header.  Every run that reads the tables
 * is over before they are written, and the write is over when the call returns.  Batches created on the context
 * before the call can simply be run again for the next iteration -- no table derivation, no upload: the wave
 * kernels' track, which carries the bin's five logs per column, is rebuilt from the context's current table at every
 * run, and the general kernel reads the table itself. */
int cpecan_hip_modelsv_set_skip_probs(cpecan_ctx *ctx, const double *skip_probs /*[60]: beta[30] | alpha[30]*/);

/* The echelon signal machine: getStateMachineEchelon() (impl/stateMachine.c:1773) after emissions_signal_scaleModel().
 * Fields as in struct _StateMachineEchelon (inc/stateMachine.h:233-246): the two end values (used as log values, as the
 * reference does), the match and extra-event tables in the reference's layout and the 60 skip-bin values of
 * EMISSION_GAP_X_PROBS (beta[30] | alpha[30]).  X elements are read as sequence_getKmer2 does; k-mers must be
 * ACGT-only.  Ids live in their own space (used by cpecan_hip_batch_create_echelon only). */
typedef struct {
    double end_match_prob, end_from_x_prob;
    const double *match_probs; /* [CPECAN_MODEL_TABLE_LEN] */
    const double *skip_probs;  /* [60]                     */
    const double *gap_y_probs; /* [CPECAN_MODEL_TABLE_LEN] */
} cpecan_echelon_model;
int cpecan_hip_modelse_create(cpecan_ctx *ctx, const cpecan_echelon_model *models, int32_t n, int32_t *ids);

/* The 3-state HDP signal machine: getHdpStateMachine3(NanoporeHDP *) (impl/stateMachine.c:1738) over a
 * finalized NanoporeHDP (deserialize_nhdp impl/nanopore_hdp.c:845).  transitions as cpecan_sm3_model; the
 * HDP as densities need it (dir_proc_density impl/hdp.c:2577-2601): the alphabet (sorted, as the k-mer ids
 * are taken over it, impl/nanopore_hdp.c:348-380), the sampling grid, and per k-mer id the row -- in
 * posterior_predictive / spline_slopes, rows x grid_length doubles -- of the Dirichlet process's nearest
 * OBSERVED ancestor.  Ids live in their own space (used by cpecan_hip_batch_create_hdp only); all models of
 * a context must share one alphabet; a model's tables hold at most 2^32 - 1 values (n_rows x grid_length: the
 * register-resident kernels index them with 32 bits), a larger one is refused with CPECAN_EINVAL. */
typedef struct {
    double transitions[9];
    const char *alphabet;
    int32_t alphabet_size;      /* <= 16 */
    int32_t grid_length;
    const double *grid;         /* [grid_length] */
    int64_t n_rows;
    const double *posterior_predictive; /* [n_rows * grid_length] */
    const double *spline_slopes;        /* [n_rows * grid_length] */
    const int32_t *kmer_row;    /* [alphabet_size ^ 6] */
} cpecan_hdp_model;
int cpecan_hip_modelsh_create(cpecan_ctx *ctx, const cpecan_hdp_model *models, int32_t n, int32_t *ids);

/* ---- band / split geometry (host integer code, exported because the reference exports it) ----
 * cpecan_band_construct: band_construct (impl/pairwiseAligner.c:132); xmyL/xmyR hold lX+lY+1 entries.
 * cpecan_split_points: getSplitPoints (:1313); out holds up to cap 4-tuples; returns the count. */
int cpecan_band_construct(const int64_t *anchors, int64_t n_anchors, int64_t lX, int64_t lY,
                          int64_t expansion, int32_t *xmyL, int32_t *xmyR);
int64_t cpecan_split_points(const int64_t *anchors, int64_t n_anchors, int64_t lX, int64_t lY,
                            int64_t max_matrix_size, int ragged_left, int ragged_right,
                            int64_t *out, int64_t cap);
/* What the kernel choice asks about an item's band, without a batch and without a device: *max_width receives the cells
 * of the widest diagonal of the band that cpecan_band_construct builds from these arguments, *edges_step_by_one 1 if
 * both edges of that band move by at most one k-mer (and never back) from each diagonal to the next, otherwise 0 --
 * the two band arguments of the plan calls below, by the rule batch creation itself applies (one piece of code).  Either
 * may be NULL.  Returns what the band's construction returns. */
int cpecan_band_extent(const int64_t *anchors, int64_t n_anchors, int64_t lX, int64_t lY, int64_t expansion,
                       int32_t *max_width, int32_t *edges_step_by_one);

/* ---- batch ---------------------------------------------------------------------------------
 * One work item = one getPosteriorProbsWithBanding() call (impl/pairwiseAligner.c:870): a k-mer
 * sequence X of lX elements (lX+5 nucleotides starting at x_chars[x_offset]), an event sequence Y
 * of lY elements (events[3*(y_offset+i)] = mean, noise, duration -- the reference's layout),
 * anchors relative to the item, ragged-end flags and a model.  Sub-alignments produced by
 * getSplitPoints are separate items that point into the same buffers. */
typedef struct {
    int64_t x_offset, lX;
    int64_t y_offset, lY;
    int64_t anchor_offset, n_anchors; /* into anchors[] as (x,y) pairs */
    int32_t model_id;
    int32_t ragged_left, ragged_right;
    int32_t reserved;
} cpecan_item;

/* the PairwiseAlignmentParameters fields this path reads (inc/pairwiseAligner.h:80-91) */
typedef struct {
    double threshold;
    int64_t minDiagsBetweenTraceBack;
    int64_t traceBackDiagonals;
    int64_t diagonalExpansion;
} cpecan_band_params;

#define CPECAN_MODE_POSTERIOR 0    /* diagonalCalculationPosteriorMatchProbs (:756) */
#define CPECAN_MODE_EXPECTATIONS 1 /* diagonalCalculation_Expectations (:841)       */

#define CPECAN_KERNEL_AUTO 0
#define CPECAN_KERNEL_GENERAL 1  /* any band width; diagonals live in HBM            */
#define CPECAN_KERNEL_SYSTOLIC 2 /* band <= 248 k-mers wide (<= 504 with a CPECAN_FLAG_WIDE_BANDS* flag); register-resident wavefront */

#define CPECAN_FLAG_DEBUG_DUMP 1 /* keep forward/backward cells for cpecan_hip_batch_debug_cells */
#define CPECAN_FLAG_UNBANDED 2   /* getAlignedPairsWithoutBanding (:1512): full matrix, one traceback from
                                    the last diagonal, one totalProbability taken there; anchors and
                                    diagonalExpansion are ignored (general kernel only) */
#define CPECAN_FLAG_SCAN_DECODE 4 /* systolic kernel, diagnostic: decode posteriors by scanning every cell of
                                    the band instead of the sweep's candidate lists (the path a window falls
                                    back to by itself when its totals drift or a list overflows) */

#define CPECAN_FLAG_EXPECTATIONS 8 /* cpecan_hip_batch_create_dna / _vanilla / _hdp: run diagonalCalculation_Expectations
                                      (:841) instead of the posterior decode, as CPECAN_MODE_EXPECTATIONS does
                                      for the signal batches */

#define CPECAN_FLAG_WORKGROUP_KERNELS 16 /* register-resident path: run this batch on the workgroup-per-alignment
                                           kernels (cpecan_k_sy_*: 1..4 waves share an alignment through LDS) instead
                                           of the wave-per-alignment ones (cpecan_k_wv_*, the default).  Same results
                                           bit for bit; the workgroup family is the one that runs several batches at
                                           once well (more, smaller-footprint workgroups per CU).  The environment
                                           variable CPECAN_KERNELS=systolic asks the same for every batch. */

#define CPECAN_FLAG_SMALL_FOOTPRINT 64 /* a batch that may run the assembly sweeps keeps the two-window ring and the single
                                        * scratch of the compiled wave kernels (24 instead of 45 GB for 1024 reads of
                                        * 10k events x 5k k-mers): its post kernel then runs between its backward sweeps
                                        * (-10 % when batches are chained, nothing for a batch alone).  For callers that
                                        * keep several one-shot batches alive at once. */
#define CPECAN_FLAG_GENERAL_KERNEL 32 /* cpecan_hip_batch_create_hdp / _vanilla: keep the batch on the general kernel
                                         (any band width) instead of the wave-per-alignment kernels of that machine
                                         (posterior decode; bands <= 248 k-mers for the HDP machine, <= 184 for the
                                         vanilla one); same results bit for bit on reads of ACGT (an HDP column that
                                         is no k-mer scores NaN here and -inf on the wave builds; a vanilla batch with
                                         one runs here anyway, see cpecan_hip_batch_create_vanilla) */
#define CPECAN_FLAG_WIDE_BANDS 128 /* cpecan_hip_batch_create (strawMan machine, posterior decode and expectations): a
                                      batch whose widest band is 249..504 k-mers runs on the six- or eight-wave build of
                                      the workgroup-per-alignment kernels (up to 376, up to 504) instead of the general
                                      kernel, whichever family is the default; CPECAN_KERNEL_SYSTOLIC then refuses
                                      only bands above 504.  A batch of narrower bands runs exactly what it runs
                                      without the flag, one of wider bands goes to the general kernel as before.
                                      cpecan_hip_batch_create_vanilla (posterior decode only): a batch whose widest band
                                      is 185..504 k-mers, past that machine's wave builds, runs on the vanilla builds of
                                      the same kernels with four, six or eight waves per workgroup (up to 248, 376, 504)
                                      unless it is un-banded or carries CPECAN_FLAG_GENERAL_KERNEL; a vanilla batch of
                                      CPECAN_MODE_EXPECTATIONS ignores the flag (its E-step past 184 k-mers runs on the
                                      general kernel, or with CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP on the E-step builds
                                      of the same kernels), and so does a vanilla batch that meets a k-mer that is none (see
                                      cpecan_hip_batch_create_vanilla), and so do the other machines.  Same results bit
                                      for bit.  The
                                      environment variable CPECAN_WIDE_BANDS=1 (read per batch) sets it for every
                                      strawMan batch and every vanilla posterior batch: the way in for callers of
                                      libcpecan_host.so and vanillaAlign. */
#define CPECAN_FLAG_WIDE_BANDS_HDP 256 /* cpecan_hip_batch_create_hdp (posterior decode only): a batch whose widest band is
                                          249..504 k-mers, past the HDP machine's wave builds, runs on the HDP builds of the
                                          workgroup-per-alignment kernels with six or eight waves per workgroup (up to
                                          376, up to 504) instead of the general kernel, unless it is un-banded, carries
                                          CPECAN_FLAG_GENERAL_KERNEL or has band edges that step by more than one k-mer.
                                          A batch of narrower bands runs on the wave builds as without the flag, one of
                                          wider bands on the general kernel as before.  An HDP batch of
                                          CPECAN_FLAG_EXPECTATIONS ignores the flag (its E-step past 248 k-mers runs on
                                          the general kernel, or with CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP on the E-step
                                          builds of the same kernels), and so do all other machines; CPECAN_FLAG_WIDE_BANDS
                                          in turn means nothing to an HDP batch.  Same results bit for bit.  The environment
                                          variable CPECAN_WIDE_BANDS_HDP=1 (read per batch) sets it for every HDP posterior
                                          batch: the way in for callers of libcpecan_host.so and vanillaAlign. */
#define CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP 512 /* cpecan_hip_batch_create_hdp with CPECAN_FLAG_EXPECTATIONS only: a batch
                                          whose widest band is 249..504 k-mers, past the HDP machine's wave builds, runs
                                          its E-step on the E-step builds of the workgroup-per-alignment kernels with six
                                          or eight waves per workgroup (up to 376, up to 504: the forward sweep keeping
                                          every state, the sweep back leaving its cells in a ring, one expectation
                                          kernel per window) instead of the general kernel, unless it carries
                                          CPECAN_FLAG_GENERAL_KERNEL or has band edges that step by more than one k-mer
                                          (an un-banded E-step is refused as without the flag).  A batch of narrower
                                          bands runs on the wave builds as without the flag, one of wider bands on the
                                          general kernel as before.  An HDP posterior batch ignores the flag, and so do
                                          all other machines; CPECAN_FLAG_WIDE_BANDS and CPECAN_FLAG_WIDE_BANDS_HDP in turn
                                          mean nothing to an HDP E-step.  The event-to-k-mer assignments are the general
                                          kernel's bit for bit, in the reference's order; the ten sums are atomic
                                          additions of the same terms and agree to rounding (as between any two runs).
                                          The environment variable CPECAN_WIDE_BANDS_HDP_ESTEP=1 (read per batch) sets it
                                          for every HDP batch of expectations: the way in for callers of
                                          libcpecan_host.so (cpecan_getHdpExpectationsUsingAnchors, cpecan_trainModels)
                                          and vanillaAlign.  One flag for the wide builds of every machine and mode is a
                                          follow-up: tests pin what the two older flags do not mean. */
#define CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP 1024 /* cpecan_hip_batch_create_vanilla with CPECAN_FLAG_EXPECTATIONS only: a
                                          batch whose widest band is 185..504 k-mers, past the vanilla machine's wave
                                          builds, runs its E-step on the vanilla E-step builds of the
                                          workgroup-per-alignment kernels with four, six or eight waves per workgroup (up
                                          to 248, 376, 504: the forward sweep keeping every state, the sweep back leaving
                                          B.gapX of its cells in a ring, one expectation kernel per window) instead of the
                                          general kernel, unless it carries CPECAN_FLAG_GENERAL_KERNEL, has band edges
                                          that step by more than one k-mer or meets a k-mer that is none (see
                                          cpecan_hip_batch_create_vanilla; an un-banded E-step is refused as without the
                                          flag).  A batch of narrower bands runs on the wave builds as without the flag,
                                          one of wider bands on the general kernel as before.  A vanilla posterior batch
                                          ignores the flag, and so do all other machines.  The 61 sums are atomic
                                          additions of the same terms as on the other kernels and agree to rounding (as
                                          between any two runs).  The environment variable
                                          CPECAN_WIDE_BANDS_VANILLA_ESTEP=1 (read per batch) sets it for every vanilla
                                          batch of expectations: the way in for callers of libcpecan_host.so
                                          (cpecan_trainModels) and vanillaAlign.  It has a number of its own because
                                          tests pin that 128, 256 and 512 mean nothing to a vanilla E-step. */
#define CPECAN_FLAG_WORKGROUP_FUSED_ESTEP 2048 /* cpecan_hip_batch_create (strawMan machine) with
                                          CPECAN_MODE_EXPECTATIONS only: a batch that runs on the workgroup-per-alignment
                                          kernels with one to four waves per workgroup (CPECAN_FLAG_WORKGROUP_KERNELS or
                                          CPECAN_KERNELS=systolic, bands up to 248 k-mers) sums its Baum-Welch
                                          expectations inside the sweep back, on the fused build of as many waves
                                          (cpecan_k_sy_backward_f1.._f4), as the wave kernels do by default: no ring of
                                          backward cells (ring diagonals x waves x 3 x 64 doubles per alignment), no
                                          expectation kernel.  The terms of a window are taken against an estimate of
                                          its total and scaled to the exact totals after the sweep; a window whose
                                          estimate is not finite or lies more than 30 nats from one of them is swept
                                          back once more in the same launch (CPECAN_EXPECT_RESWEEP=1 sends every window
                                          there, =2 every other one: tests).  The kernel choice does not change:
                                          cpecan_hip_plan_dispatch answers what it answers without the flag
                                          (cpecan_hip_plan_expectation_pass tells what the flag does), and every
                                          other batch -- a posterior batch, another machine, the wave kernels, the six-
                                          and eight-wave builds of CPECAN_FLAG_WIDE_BANDS, the general kernel -- ignores
                                          it.  The sums are those of the other E-step paths to rounding (the same terms
                                          in another order, scaled once per segment of ten diagonals), NaN in the same
                                          places.  Opt-in: the fused sweep back holds 174-177 VGPRs against 125-127, so
                                          two waves run per SIMD where four did.  Measured: a batch
                                          alone runs 1.02x, 1.11x and 1.36x as fast at two, three and four waves per
                                          workgroup, bench.py --mode em 1.05x (four and two contexts, three waves) --
                                          and SLOWER, 0.90x, at one wave per workgroup (bands up to 56 k-mers): leave
                                          the flag off for such batches.  The environment
                                          variable CPECAN_EXPECT_FUSED_WORKGROUP=1 (read per batch) sets it for every
                                          strawMan batch of expectations: the way in for callers of libcpecan_host.so
                                          (cpecan_trainModels) and for em.PersistentEStep. */
#define CPECAN_FLAG_WIDE_BANDS_FUSED_ESTEP 4096 /* cpecan_hip_batch_create (strawMan machine) with
                                          CPECAN_MODE_EXPECTATIONS only: a batch that the kernel choice put on the six-
                                          or eight-wave build of the workgroup-per-alignment kernels (CPECAN_FLAG_WIDE_BANDS
                                          or CPECAN_WIDE_BANDS=1, a widest band of 249..504 k-mers) sums its Baum-Welch
                                          expectations inside the sweep back, on the fused build of as many waves
                                          (cpecan_k_sy_backward_f6 / _f8), as CPECAN_FLAG_WORKGROUP_FUSED_ESTEP does up
                                          to four waves: no ring of backward cells (ring diagonals x 6 or 8 x 3 x 64
                                          doubles per alignment, 9 or 12 KB per diagonal), no expectation kernel; the
                                          estimate, the scaling, the second sweep and CPECAN_EXPECT_RESWEEP are those
                                          described there.  The kernel choice does not change: cpecan_hip_plan_dispatch
                                          answers what it answers without the flag (cpecan_hip_plan_expectation_pass
                                          tells what the flag does).  Every other batch ignores it: a
                                          posterior batch, a band of 248 k-mers or less (flag 2048's ground), a band
                                          past 504 k-mers and a wide band without CPECAN_FLAG_WIDE_BANDS (both on the
                                          general kernel), every other machine.  It has a number of its own because a
                                          test pins that 2048 | 128 keeps the ring of backward cells at six waves.
                                          The sums are those of the ring path to rounding, NaN in the same places.
                                          Opt-in.  The eight-wave fused sweep back holds 179 VGPRs against 127, so one
                                          workgroup runs per CU where two did; the six-wave one keeps its eight sums in
                                          LDS and fits three waves per SIMD (165 VGPRs), two workgroups per CU as before.
                                          Measured: a batch alone runs 1.36x as fast at eight
                                          waves per workgroup (bands of 377..504 k-mers) -- and SLOWER, 0.97-0.98x, at
                                          six (249..376: the sweep back alone takes as long as the ring's sweep back and
                                          expectation kernel together): leave the flag off for such batches.  The
                                          environment variable
                                          CPECAN_EXPECT_FUSED_WIDE=1 (read per batch) sets it for every strawMan batch of
                                          expectations: the way in for callers of libcpecan_host.so (cpecan_trainModels),
                                          vanillaAlign and em.PersistentEStep, together with CPECAN_WIDE_BANDS=1. */
#define CPECAN_FLAG_ASM_NARROW_BANDS 8192 /* cpecan_hip_batch_create (strawMan machine) with CPECAN_MODE_POSTERIOR
                                          only: a batch of the wave-per-alignment kernels whose widest band is at most
                                          120 k-mers -- two cells per lane, the ground of the _l2 build: what the
                                          reference's default diagonalExpansion of 20 and its driver's 50 give (bands of
                                          about 72 and 102 k-mers around anchors every 50 columns) -- runs the
                                          hand-scheduled assembly sweeps at two cells per lane
                                          (cpecan_k_asm_forward_l2 / cpecan_k_asm_backward_l2) in place of the compiled
                                          sweeps of that build, with everything a three-cell assembly batch has: the
                                          three-window ring (CPECAN_FLAG_SMALL_FOOTPRINT: the two-window one), the lane
                                          sets, the compiled post and re-sweep kernels, the compiled kernels when a
                                          set-up launch fails, under CPECAN_ASM=0 or when the model lets gap Y switch to
                                          gap X.  cpecan_hip_batch_assembly_sweeps reports 2,
                                          cpecan_hip_plan_assembly_sweeps answers beforehand; the kernel, family and
                                          build cpecan_hip_plan_dispatch names do not change.  Results are bit-identical
                                          to the compiled kernels': pairs, their order, posteriors, totals.  Every other
                                          batch ignores the flag: another machine, a batch of expectations, the
                                          workgroup-per-alignment family (CPECAN_FLAG_WORKGROUP_KERNELS,
                                          CPECAN_KERNELS=systolic), the general kernel, a band of 121 k-mers or more
                                          (121..158 run the three-cell assembly sweeps with or without it).  Opt-in:
                                          tests pin that such a batch without the flag runs the compiled sweeps.  The
                                          environment variable CPECAN_ASM_NARROW=1 (read per batch) sets it for every
                                          strawMan posterior batch: the way in for callers of libcpecan_host.so,
                                          vanillaAlign and bench.py --band. */
#define CPECAN_FLAG_VANILLA_FUSED_ESTEP 16384 /* cpecan_hip_batch_create_vanilla with CPECAN_FLAG_EXPECTATIONS only: a
                                          batch of the wave-per-alignment kernels (a widest band of at most 184 k-mers
                                          whose edges step by one k-mer per diagonal, no CPECAN_FLAG_GENERAL_KERNEL) sums
                                          its two expectations per cell -- match -> gap X into the skip bin of the cell's
                                          k-mer pair, gap X -> gap X into bin + 30 -- inside the sweep back, against the
                                          forward sweep's estimate of the window's total, per segment of ten decoded
                                          diagonals (cpecan_k_wv_backward_fx_vf2 / _vf3, on the build of as many cells
                                          per lane as the batch would run on without the flag): no ring of backward
                                          cells, no expectation kernel.  The post kernel scales a segment's sums by
                                          exp(estimate - total); a window whose estimate is not finite or lies more than
                                          30 nats from one of its totals is swept once more against the exact totals
                                          (CPECAN_EXPECT_RESWEEP=1 / 2 forces that for every / every other window:
                                          tests).  cpecan_hip_batch_expectation_pass reports 1,
                                          cpecan_hip_plan_expectation_pass answers beforehand; the kernel, family, rows
                                          and widest band cpecan_hip_plan_dispatch names do not change.  Results agree
                                          with the ring path to rounding (the sums are added in another order).  These
                                          builds have no other form of the E-step: CPECAN_EXPECT_FUSED=0 does not undo
                                          the flag.  Every other batch ignores it: a posterior batch, another machine,
                                          a vanilla E-step on the general kernel (CPECAN_FLAG_GENERAL_KERNEL, a band
                                          past 184 k-mers, band edges that step by more than one, a k-mer that is none)
                                          or on the _ve workgroup builds (CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP, 185..504
                                          k-mers).  Opt-in: tests pin that a vanilla batch of expectations without the
                                          flag keeps the ring.  No environment variable of the C-ABI sets it;
                                          libcpecan_host.so sets it for its vanilla batches of expectations when
                                          CPECAN_VANILLA_FUSED_ESTEP=1 (the way in for vanillaAlign and
                                          cpecan_trainModels). */
#define CPECAN_FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP 32768 /* cpecan_hip_batch_create_vanilla with
                                          CPECAN_FLAG_EXPECTATIONS only: a batch that CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP
                                          (or CPECAN_WIDE_BANDS_VANILLA_ESTEP=1) puts on the _ve workgroup builds -- a
                                          widest band of 185..504 k-mers whose edges step by one k-mer per diagonal, no
                                          CPECAN_FLAG_GENERAL_KERNEL, no k-mer that is none -- sums its two expectations
                                          per cell inside the sweep back instead (cpecan_k_sy_backward_vf4 / _vf6 / _vf8,
                                          the build of as many waves per workgroup), as CPECAN_FLAG_VANILLA_FUSED_ESTEP
                                          does on the wave kernels: against the sweep's estimate of the window's total,
                                          per segment of ten decoded diagonals, scaled by exp(estimate - total) after
                                          the totals, in the same launch; no ring of backward cells, no expectation
                                          kernel.  A window whose estimate is not finite or lies more than 30 nats from
                                          one of its totals is swept back once more in that launch against the exact
                                          totals (CPECAN_EXPECT_RESWEEP=1 / 2 forces that for every / every other
                                          window: tests).  cpecan_hip_batch_expectation_pass reports 1,
                                          cpecan_hip_plan_expectation_pass answers beforehand; the kernel, family, rows
                                          and widest band cpecan_hip_plan_dispatch names do not change.  Results agree
                                          with the ring path to rounding (the sums are added in another order).  These
                                          builds have no other form of the E-step: CPECAN_EXPECT_FUSED=0 does not undo
                                          the flag.  Every other batch ignores it: a posterior batch, another machine,
                                          a band of at most 184 k-mers (the wave kernels, where
                                          CPECAN_FLAG_VANILLA_FUSED_ESTEP rules) or past 504, the general kernel, a
                                          batch without the wide-bands flag of the E-step.  A number of its own because
                                          16384 is pinned as meaning nothing to a batch on the _ve builds.  Opt-in, and
                                          as measured so far slower than the ring path (0.81 / 0.91 / 0.96 x at four /
                                          six / eight waves: the fused sweep back takes 141..145 registers where the
                                          ring build's takes 124..128).  No
                                          environment variable of the C-ABI sets it; libcpecan_host.so sets it for its
                                          vanilla batches of expectations when CPECAN_WIDE_BANDS_VANILLA_FUSED_ESTEP=1
                                          (the way in for vanillaAlign and cpecan_trainModels, beside
                                          CPECAN_WIDE_BANDS_VANILLA_ESTEP=1). */
#define CPECAN_FLAG_HDP_FUSED_ESTEP 65536 /* cpecan_hip_batch_create_hdp with CPECAN_FLAG_EXPECTATIONS only: a batch of
                                          the wave-per-alignment kernels at two or three cells per lane (a widest band
                                          of at most 184 k-mers whose edges step by one k-mer per diagonal, no
                                          CPECAN_FLAG_GENERAL_KERNEL; a narrow band that CPECAN_SYSTOLIC_ROWS=3 puts on
                                          three cells included) sums its eight transition expectations and the
                                          likelihood inside the sweep back, against the forward sweep's estimate of the
                                          window's total, per segment of ten decoded diagonals
                                          (cpecan_k_wv_backward_fx_hf2 / _hf3, on the build of as many cells per lane as
                                          the batch would run on without the flag): no ring of backward cells, no
                                          expectation kernel.  The sweep parks every transition into match whose
                                          exponent lies within 0.25 of the threshold against the estimate; the post
                                          kernel scales a segment's sums by exp(estimate - total) and selects the
                                          assignments from that list with the exact total, so the triples and their
                                          exponents are the ring path's bit for bit, and the sums agree with it to
                                          rounding (they are added in another order).  A window with a total that is not
                                          finite or lies more than 0.25 from the estimate, whose list overflowed, or of
                                          a batch whose threshold has no logarithm, is swept once more against the exact
                                          totals, sums and assignments both (CPECAN_EXPECT_RESWEEP=1 / 2 forces that for
                                          every / every other window: tests).  cpecan_hip_batch_expectation_pass reports
                                          1, cpecan_hip_plan_expectation_pass answers beforehand; the kernel, family,
                                          rows and widest band cpecan_hip_plan_dispatch names do not change.  These
                                          builds have no other form of the E-step: CPECAN_EXPECT_FUSED=0 does not undo
                                          the flag.  Every other batch ignores it: a posterior batch, another machine,
                                          an HDP E-step at four cells per lane (bands of 185..248 k-mers: _h4 keeps its
                                          ring under this flag; CPECAN_FLAG_HDP_FOUR_CELLS_FUSED_ESTEP serves it), on the _he6 / _he8 workgroup builds (CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP,
                                          249..504 k-mers) or on the general kernel.  Opt-in: an HDP batch of
                                          expectations without the flag keeps the ring.  No environment variable of the
                                          C-ABI sets it; libcpecan_host.so sets it for its HDP batches of expectations
                                          when CPECAN_HDP_FUSED_ESTEP=1 (the way in for
                                          cpecan_getHdpExpectationsUsingAnchors, cpecan_trainModels and vanillaAlign). */
#define CPECAN_FLAG_WIDE_BANDS_HDP_FUSED_ESTEP 131072 /* cpecan_hip_batch_create_hdp with CPECAN_FLAG_EXPECTATIONS only:
                                          a batch that CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP (or
                                          CPECAN_WIDE_BANDS_HDP_ESTEP=1) puts on the _he6 / _he8 workgroup builds -- a
                                          widest band of 249..504 k-mers whose edges step by one k-mer per diagonal, no
                                          CPECAN_FLAG_GENERAL_KERNEL -- sums its eight transition expectations and the
                                          likelihood inside the sweep back instead (cpecan_k_sy_backward_hf6 / _hf8, the
                                          build of as many waves per workgroup), as CPECAN_FLAG_HDP_FUSED_ESTEP does on
                                          the wave kernels: against the sweep's estimate of the window's total, per
                                          segment of ten decoded diagonals, scaled by exp(estimate - total) after the
                                          totals, in the same launch; no ring of backward cells, no expectation kernel.
                                          The sweep parks every transition into match whose exponent lies within 0.25 of
                                          the threshold against the estimate, and a selection phase of the same launch
                                          takes the assignments from that list with the exact total, so the triples and
                                          their exponents are the ring path's bit for bit, and the sums agree with it to
                                          rounding (they are added in another order).  A window with a total that is not
                                          finite or lies more than 0.25 from the estimate, whose list overflowed, or of
                                          a batch whose threshold has no logarithm, is swept back once more in that
                                          launch against the exact totals, sums and assignments both
                                          (CPECAN_EXPECT_RESWEEP=1 / 2 forces that for every / every other window:
                                          tests).  cpecan_hip_batch_expectation_pass reports 1,
                                          cpecan_hip_plan_expectation_pass answers beforehand; the kernel, family, rows
                                          and widest band cpecan_hip_plan_dispatch names do not change.  These builds
                                          have no other form of the E-step: CPECAN_EXPECT_FUSED=0 does not undo the
                                          flag.  Every other batch ignores it: a posterior batch, another machine, a
                                          band of at most 248 k-mers (the wave kernels, where
                                          CPECAN_FLAG_HDP_FUSED_ESTEP rules up to 184) or past 504, the general kernel,
                                          a batch without the wide-bands flag of the E-step.  A number of its own
                                          because 65536 is pinned as meaning nothing to a batch on the _he builds, and
                                          keeps meaning nothing there.  Opt-in.  As measured (1024 reads of 2 000
                                          k-mers, threshold 0.05): a gain at both widths, 1.10 x the ring path at six
                                          waves (widest band 321: 52.9 against 58.0 ms) and 1.10 x at eight (441: 61.8
                                          against 68.0 ms; 1.13 x in another run).  No environment variable of the C-ABI
                                          sets it; libcpecan_host.so sets it for its HDP batches of expectations when
                                          CPECAN_WIDE_BANDS_HDP_FUSED_ESTEP=1 (the way in for
                                          cpecan_getHdpExpectationsUsingAnchors, cpecan_trainModels and vanillaAlign,
                                          beside CPECAN_WIDE_BANDS_HDP_ESTEP=1). */
#define CPECAN_FLAG_HDP_FOUR_CELLS_FUSED_ESTEP 262144 /* cpecan_hip_batch_create_hdp with CPECAN_FLAG_EXPECTATIONS only:
                                          a batch of the wave-per-alignment kernels at four cells per lane (a widest
                                          band of 185..248 k-mers whose edges step by one k-mer per diagonal, no
                                          CPECAN_FLAG_GENERAL_KERNEL; a narrower band that CPECAN_SYSTOLIC_ROWS=4 puts
                                          on four cells included) sums its eight transition expectations and the
                                          likelihood inside the sweep back and selects its assignments from the list
                                          the sweep parks, as CPECAN_FLAG_HDP_FUSED_ESTEP does at two and three cells:
                                          cpecan_k_wv_backward_fx_hf4 in place of _h4's sweep back and expectation
                                          kernel, cpecan_k_wv_post_hf4 for the totals, the scaling by
                                          exp(estimate - total) and the selection with the exact totals, no ring of
                                          backward cells.  Triples and exponents are the ring path's bit for bit, the
                                          sums agree with it to rounding.  A window with a total that is not finite or
                                          lies more than 0.25 from the estimate, whose list overflowed (4 records per
                                          ring diagonal and layer), or of a batch whose threshold has no logarithm, is
                                          swept once more against the exact totals, by cpecan_k_wv_resweep_fx_hf4;
                                          CPECAN_EXPECT_RESWEEP=1 / 2 forces that for every / every other window, for
                                          tests.  cpecan_hip_batch_expectation_pass reports 1,
                                          cpecan_hip_plan_expectation_pass answers beforehand; the kernel, family, rows
                                          (4) and widest band (248) cpecan_hip_plan_dispatch names do not change.  The
                                          build has no other form of the E-step: CPECAN_EXPECT_FUSED=0 does not undo the
                                          flag.  Every other batch ignores it: a posterior batch, another machine, an
                                          HDP E-step at two or three cells per lane (bands up to 184 k-mers, where
                                          CPECAN_FLAG_HDP_FUSED_ESTEP rules; a batch may carry both and is then fused at
                                          two, three and four cells), on the _he / _hf workgroup builds, a band past
                                          248 k-mers or with edges that step by more than one, the general kernel.  A
                                          number of its own because 65536 is pinned as meaning nothing to a batch on
                                          _h4, and keeps meaning nothing there.  Opt-in: an HDP batch of expectations
                                          without the flag keeps the ring.  As measured (1024 reads of 2 000 k-mers,
                                          threshold 0.05): a gain at both ends of the range, 1.15 x
                                          the ring path at a widest band of 196 k-mers (37.8 against 43.4 ms) and 1.34 x
                                          at 236 (39.9 against 53.3 ms), less than at two and three cells: a forward
                                          wave (232 registers) and a fused backward wave (432) do not share a SIMD, so
                                          the forward sweep beside it takes 6.7..7.1 ms a window instead of 4.6..5.4.
                                          No environment variable of the
                                          C-ABI sets it; libcpecan_host.so sets it for its HDP batches of expectations
                                          when CPECAN_HDP_FOUR_CELLS_FUSED_ESTEP=1 (the way in for
                                          cpecan_getHdpExpectationsUsingAnchors, cpecan_trainModels and vanillaAlign). */
#define CPECAN_FLAG_SM4_WAVE 524288 /* cpecan_hip_batch_create_sm4 only: a banded batch whose widest band is at most 128
                                          cells (no CPECAN_FLAG_UNBANDED, no CPECAN_FLAG_GENERAL_KERNEL) runs on the
                                          one-wave-per-alignment kernels of the 4-state machine, cpecan_k_wave4_l1
                                          for bands up to 64 cells at one cell per lane, cpecan_k_wave4_l2 for 65..128
                                          at two:
                                          the recurrence in registers, one lane shift per diagonal, the traceback
                                          windows swept back in the same launch (cpecan_kernel_wave4.hip), in place of
                                          cpecan_k_general4's workgroup per alignment with its diagonals in HBM behind
                                          a barrier.  Band edges may step by any number of k-mers.  Totals, exponents
                                          and pairs are the general kernel's bit for bit; buffers, readback, chaining
                                          and the threshold-0 re-run are those of any batch.  A wider or un-banded
                                          batch with the flag runs on cpecan_k_general4 as without it.
                                          cpecan_hip_plan_dispatch and cpecan_hip_batch_kernel_family report such a
                                          batch as they report a DNA batch on the 5-state wave kernels: kernel GENERAL,
                                          wave 1, rows 0; cpecan_hip_batch_info keeps saying general.  Every other
                                          machine ignores the flag.  Opt-in: without it nothing changes.  No
                                          environment variable of the C-ABI sets it; libcpecan_host.so sets it for its
                                          4-state posterior batches when CPECAN_SM4_WAVE=1 (the way in for
                                          getAlignedPairsUsingAnchors with a fourState machine, vanillaAlign --fourState
                                          and the stream).  As measured (2 000 k-mers x 4 000 events, the two ways run in
                                          turn on one box): 1.50 x the general kernel at 1024
                                          alignments with the driver's diagonalExpansion of 50 (widest band 105: 69.1
                                          against 103.4 ms) and 2.25 x at a band of 63 (37.1 against 83.3 ms); 2.58 x
                                          and 3.70 x at 4096 alignments (168.3 against 434.7 ms, 93.4 against 345.5). */

/* Copies the inputs to HBM and builds per-item band tables.  All host pointers may be released
 * after the call returns. */
int cpecan_hip_batch_create(cpecan_ctx *ctx, const cpecan_item *items, int64_t n_items,
                            const char *x_chars, int64_t n_x_chars, const double *events,
                            int64_t n_events, const int64_t *anchors, int64_t n_anchor_pairs,
                            const cpecan_band_params *params, int32_t mode, int32_t kernel,
                            int32_t flags, cpecan_batch **batch);
/* Runs the DP for every item (asynchronous on the context's stream). */
/* DNA against DNA with a 5-state model (getAlignedPairsUsingAnchors with a stateMachine5 and
 * sequence_getBase on both sides, impl/pairwiseAligner.c:1456,:308): X and Y are nucleotide strings,
 * lX / lY count bases, x_offset / y_offset index x_chars / y_chars, model_id is a
 * cpecan_hip_models5_create id.  General kernel; flags: DEBUG_DUMP is not available, UNBANDED and
 * EXPECTATIONS are (the latter: hmmDiscrete sums through cpecan_hip_batch_fetch_expectations). */
int cpecan_hip_batch_create_dna(cpecan_ctx *ctx, const cpecan_item *items, int64_t n_items,
                                const char *x_chars, int64_t n_x, const char *y_chars, int64_t n_y,
                                const int64_t *anchors, int64_t n_anchor_pairs,
                                const cpecan_band_params *params, int32_t flags, cpecan_batch **out);

/* k-mers against events with a vanilla model (getAlignedPairsUsingAnchors with a StateMachine3Vanilla,
 * sequence_getKmer2 / sequence_getEvent): same buffers as cpecan_hip_batch_create, model_id is a
 * cpecan_hip_modelsv_create id.  flags: UNBANDED (general kernel, posterior decode only), EXPECTATIONS, GENERAL_KERNEL,
 * WIDE_BANDS, WIDE_BANDS_VANILLA_ESTEP, VANILLA_FUSED_ESTEP, WIDE_BANDS_VANILLA_FUSED_ESTEP.  There is no kernel argument: the batch picks its kernels itself (the wave builds
 * up to 184 k-mers of band, the general kernel past that), and the two wide-bands flags alone select the workgroup builds
 * for bands of 185..504 k-mers: CPECAN_FLAG_WIDE_BANDS for the posterior decode, CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP for
 * the E-step.
 * One exception, whatever the flags: a batch in which any item has a character outside ACGT among its lX + 5, or fewer
 * than two k-mers (lX < 2: sequence_getKmer2 looks one k-mer ahead, past such an item's end), runs as a whole on the
 * general kernel.  The reference scores a k-mer that is none as NaN under this machine and NaN spreads through its
 * logAdd; the general kernel reproduces that bit for bit, the register-resident kernels cannot (their branch-free
 * logAdd drops a NaN operand).  One such read moves its whole batch: callers that care for the speed of the others
 * put reads with foreign characters into a batch of their own (the general kernel is several times slower than
 * the wave kernels; what the move costs a vanilla batch has not been measured).  cpecan_hip_batch_info reports the
 * kernel. */
int cpecan_hip_batch_create_vanilla(cpecan_ctx *ctx, const cpecan_item *items, int64_t n_items,
                                    const char *x_chars, int64_t n_x, const double *events, int64_t n_events,
                                    const int64_t *anchors, int64_t n_anchor_pairs,
                                    const cpecan_band_params *params, int32_t flags, cpecan_batch **out);

/* k-mers against events with a 4-state model (getAlignedPairsUsingAnchors / getAlignedPairsWithoutBanding with the
 * StateMachine of getStateMachine4, sequence_getKmer / sequence_getEvent): same buffers as cpecan_hip_batch_create,
 * model_id is a cpecan_hip_models4_create id.  General kernel, posterior decode; flags: UNBANDED. */
int cpecan_hip_batch_create_sm4(cpecan_ctx *ctx, const cpecan_item *items, int64_t n_items,
                                const char *x_chars, int64_t n_x, const double *events, int64_t n_events,
                                const int64_t *anchors, int64_t n_anchor_pairs,
                                const cpecan_band_params *params, int32_t flags, cpecan_batch **out);

/* k-mers against events with an echelon model (getAlignedPairsUsingAnchors / getAlignedPairsWithoutBanding with the
 * StateMachine of getStateMachineEchelon and diagonalCalculationMultiPosteriorMatchProbs, sequence_getKmer2 /
 * sequence_getEvent): same buffers as cpecan_hip_batch_create, model_id is a cpecan_hip_modelse_create id.  General
 * kernel, posterior decode; flags: UNBANDED.  A cell emits s pairs (x+n-1, y-1), n < s, for every state s = 1..5 whose
 * posterior reaches the threshold (impl/pairwiseAligner.c:797-839), so pairs repeat and x may reach lX+3.  The
 * machine looks up to 30 characters past an item's lX+5 (emissions_signal_multipleKmerMatchProb): an item's
 * `reserved` holds how many characters after those belong to its sequence (0..30; a sub-alignment of a longer read
 * sees the rest of the read), and every character past them reads as the pad 'n' of sequence_padSequence. */
int cpecan_hip_batch_create_echelon(cpecan_ctx *ctx, const cpecan_item *items, int64_t n_items,
                                    const char *x_chars, int64_t n_x, const double *events, int64_t n_events,
                                    const int64_t *anchors, int64_t n_anchor_pairs,
                                    const cpecan_band_params *params, int32_t flags, cpecan_batch **out);

/* k-mers against events with an HDP model (getAlignedPairsUsingAnchors with a StateMachine3_HDP,
 * sequence_getKmer3 / sequence_getEvent): same buffers as cpecan_hip_batch_create (x characters over the
 * model's alphabet), model_id is a cpecan_hip_modelsh_create id.  flags: UNBANDED (general kernel, posterior decode
 * only), EXPECTATIONS, GENERAL_KERNEL, WIDE_BANDS_HDP, WIDE_BANDS_HDP_ESTEP, HDP_FUSED_ESTEP, WIDE_BANDS_HDP_FUSED_ESTEP,
 * HDP_FOUR_CELLS_FUSED_ESTEP.  There is no kernel argument: the batch picks
 * its kernels itself (the HDP wave builds up to 248 k-mers of band, the general kernel past that), and the two
 * wide-bands flags alone select the workgroup builds for bands of 249..504 k-mers: CPECAN_FLAG_WIDE_BANDS_HDP for the
 * posterior decode, CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP for the E-step.  cpecan_hip_batch_info reports the kernel. */
int cpecan_hip_batch_create_hdp(cpecan_ctx *ctx, const cpecan_item *items, int64_t n_items,
                                const char *x_chars, int64_t n_x, const double *events, int64_t n_events,
                                const int64_t *anchors, int64_t n_anchor_pairs,
                                const cpecan_band_params *params, int32_t flags, cpecan_batch **out);

int cpecan_hip_batch_run(cpecan_batch *batch);
/* The same, but ordered on the device behind the last run of `after` (a batch on the same device; NULL, the batch
 * itself or a batch that has never run: no condition), with no host round trip.
 * Every run goes on a lane set: three streams (forward sweeps; sweeps back; post kernels, counts and pair packing).
 * Each context has one; a run with no condition uses its own context's.
 * What is ordered:
 *  - `after` ran on the wave-per-alignment kernels as one stream group: this run is issued on the lane set `after`
 *    ran on, behind it on each of the three streams.  Its first kernel starts when `after`'s last forward sweep has
 *    finished; its sweeps back queue behind `after`'s sweeps back, its post kernels, counts and packing behind
 *    `after`'s.  A chain of such batches uses the three streams of its first batch's lane set, whatever the number of
 *    batches and contexts in it: it fits the runtime's default of four hardware queues.
 *  - otherwise: this run starts, on its own context's lane set, when `after`'s whole run has finished.
 *  - always: this run starts after the batch's own previous run has finished, wherever that one went.
 * What is not ordered: nothing says that `after` has finished when this run has.  `after`'s results are read through
 * `after`'s own cpecan_hip_batch_sync or readback (counts, pairs, totals), which wait for `after`'s run alone and not
 * for the lanes it went on.  Runs of two host threads onto one lane set are queued whole, one after the other; a batch
 * itself (and a context) is used by one thread at a time.  A run holds its lane set until the batch runs again or is
 * destroyed, so `after`'s context may be destroyed while this run goes on.
 * A stream of batches then keeps the device busy with one pass at a time (the wave-per-alignment kernels fill the
 * register files with one batch) while the host fetches and finishes the previous batch's pairs and prepares the next
 * one. */
int cpecan_hip_batch_run_after(cpecan_batch *batch, cpecan_batch *after);
int cpecan_hip_batch_sync(cpecan_batch *batch);
/* HIP-event time of the last run's kernels, in ms (after sync). */
int cpecan_hip_batch_elapsed_ms(cpecan_batch *batch, float *ms_total, float *ms_dp_kernel);
/* The shader clock (MHz) the chip ran at during the forward sweeps of the batch's last run, from the sweeps' own cycle
 * and 100 MHz reference counters (wave-per-alignment kernels; 0 on the other kernels).  The sweeps are bound by
 * instruction issue, so their time follows this clock, and it differs between machines under this fp64 load. */
int cpecan_hip_batch_shader_clock_mhz(cpecan_batch *batch, double *mhz);
/* Which kernel the batch uses (CPECAN_KERNEL_GENERAL / _SYSTOLIC after AUTO is resolved), how many
 * workgroups it launches and the widest band (cells) among its items. */
int cpecan_hip_batch_info(cpecan_batch *batch, int32_t *kernel, int32_t *workgroups, int32_t *max_width);
/* The device memory the batch holds now: the sum of its blocks, each at the size the allocator handed it out.  It grows
 * where a run or a readback grows an output capacity; it is part of its context's figure (the ctx memory call above). */
int cpecan_hip_batch_device_bytes(cpecan_batch *batch, int64_t *bytes);
/* The machines of the create calls above, in the order of: cpecan_hip_batch_create, _dna, _vanilla, _hdp, _sm4, _echelon. */
#define CPECAN_MACHINE_STRAWMAN 0
#define CPECAN_MACHINE_DNA5 1
#define CPECAN_MACHINE_VANILLA 2
#define CPECAN_MACHINE_HDP 3
#define CPECAN_MACHINE_SM4 4
#define CPECAN_MACHINE_ECHELON 5
/* The kernel choice of batch creation, without a batch and without a device: what a batch of that machine, mode
 * (CPECAN_MODE_*; the create calls that take CPECAN_FLAG_EXPECTATIONS turn it into the mode), requested kernel (the
 * strawMan machine's; the others ignore it) and flags would run on if its widest band were max_width cells and its band
 * edges did (1) or did not (0) all move by at most one k-mer per diagonal.  Reads the environment as batch creation
 * does.  *kernel_out: as batch_info reports it; *wave_out, *rows_out: as batch_kernel_family and batch_systolic_rows
 * do (rows 0 on the general kernel); *build_max_width_out: the widest band the chosen build takes (0 on the general
 * kernel).  Any of the four may be NULL.  A combination batch creation refuses is refused here with the same code and
 * last_error. */
int cpecan_hip_plan_dispatch(int32_t machine, int32_t mode, int32_t kernel, int32_t flags, int32_t max_width,
                             int32_t edges_step_by_one, int32_t *kernel_out, int32_t *wave_out, int32_t *rows_out,
                             int32_t *build_max_width_out);
/* The same question about the hand-scheduled assembly sweeps, answered as batch creation would before it knows the
 * device (one stream group and a module that loads are left to set-up): returns 0 if such a batch would run the
 * compiled sweeps (or the general kernel), otherwise the cells per lane of the assembly sweeps it would run -- 3 for a
 * strawMan posterior batch of the wave kernels with a widest band of 121..158 k-mers, 2 with
 * CPECAN_FLAG_ASM_NARROW_BANDS or CPECAN_ASM_NARROW=1 for one of at most 120 -- and stores the same number in
 * *cells_per_lane_out (may be NULL).  Reads the environment as batch creation does (CPECAN_ASM=0: 0).  A combination
 * batch creation refuses gives 0 here, with the refusal in last_error. */
int cpecan_hip_plan_assembly_sweeps(int32_t machine, int32_t mode, int32_t kernel, int32_t flags, int32_t max_width,
                                    int32_t edges_step_by_one, int32_t *cells_per_lane_out);
/* Systolic path only: waves per workgroup of the kernel build the batch runs on -- the fewest whose 64 slots each
 * hold the widest band of the batch: 1 (bands up to 56 k-mers), 2 (120), 3 (184) or 4 (248).  The fewer waves an
 * alignment takes, the more alignments a CU holds (16, 8, 5, 4).  With CPECAN_FLAG_WIDE_BANDS also 6 (bands of 249..376
 * k-mers) and 8 (377..504): the wide builds, two workgroups per CU; for a vanilla batch with that flag 4 (185..248), 6
 * and 8, and the same three for a vanilla batch of expectations with CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP. */
int cpecan_hip_batch_systolic_rows(cpecan_batch *batch, int32_t *rows);
/* Register-resident path only: *wave = 1 if the batch runs on the wave-per-alignment kernels (rows is then the
 * number of cells a lane holds: 2, 3 or 4), 0 on the workgroup-per-alignment ones (rows = waves per workgroup).  For a
 * DNA batch: 1 if its posterior decode runs on the one-wave-per-alignment 5-state kernel (bands up to 192 cells), 0 if
 * on the general one.  For a 4-state batch: 1 if it runs on the one-wave-per-alignment 4-state kernel
 * (CPECAN_FLAG_SM4_WAVE, bands up to 128 cells), 0 if on the general one. */
int cpecan_hip_batch_kernel_family(cpecan_batch *batch, int32_t *wave);
/* *sweeps = 1 if the batch's sweeps run on the hand-scheduled assembly kernels (strawMan machine, posterior decode,
 * bands of 121..158 k-mers: the BASELINE configs[2] shape; with CPECAN_FLAG_ASM_NARROW_BANDS also bands of at most 120),
 * 2 if both the forward and the backward sweep do, 0 if on the compiled kernels.  CPECAN_ASM=0 in the environment keeps every batch on the compiled kernels.  A batch planned for
 * them whose setup launch failed runs on the compiled kernels: 0, and last_error says why. */
int cpecan_hip_batch_assembly_sweeps(cpecan_batch *batch, int32_t *sweeps);
/* *fused = 1 if the batch's E-step sums its Baum-Welch expectations inside the sweep back: the strawMan machine on the
 * wave kernels (CPECAN_EXPECT_FUSED=0 in the environment when the batch is created opts out) and, with
 * CPECAN_FLAG_WORKGROUP_FUSED_ESTEP or CPECAN_EXPECT_FUSED_WORKGROUP=1, on the workgroup kernels of one to four waves,
 * with CPECAN_FLAG_WIDE_BANDS_FUSED_ESTEP or CPECAN_EXPECT_FUSED_WIDE=1 on those of six and eight waves
 * (cpecan_hip_batch_kernel_family tells which), and the vanilla machine on the wave kernels (bands up to 184 k-mers)
 * with CPECAN_FLAG_VANILLA_FUSED_ESTEP and on the workgroup kernels of four, six and eight waves (185..504) with
 * CPECAN_FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP: no ring of backward cells, no expectation kernel.  0 for the
 * ring-of-backward-cells path and for posterior batches. */
int cpecan_hip_batch_expectation_pass(cpecan_batch *batch, int32_t *fused);
/* The same beforehand, without a batch and without a device, asked as cpecan_hip_plan_dispatch is: returns (and stores
 * in *fused_out, which may be NULL) what cpecan_hip_batch_expectation_pass would report for such a batch.  A combination
 * batch creation refuses gives 0 here, with the refusal in last_error. */
int cpecan_hip_plan_expectation_pass(int32_t machine, int32_t mode, int32_t kernel, int32_t flags, int32_t max_width,
                                     int32_t edges_step_by_one, int32_t *fused_out);
/* Systolic path only: HIP-event time of the last run spent in the forward-window kernels and in
 * the backward-window kernels (each launched `launches_each` times, once per traceback window). */
int cpecan_hip_batch_stage_ms(cpecan_batch *batch, float *ms_forward, float *ms_backward,
                              int32_t *launches_each);
/* Per-item result sizes: aligned pairs, refreshes of totalProbability, in-band cells. */
int cpecan_hip_batch_counts(cpecan_batch *batch, int64_t *n_pairs, int64_t *n_totals,
                            int64_t *n_cells);
/* Aligned pairs of one item as (floor(p*1e7), x, y) int64 triples in the order the reference's
 * diagonalPosteriorProbFn emits them (windows forward, diagonals descending, x-y ascending);
 * logp (may be NULL) receives (F+B)-total for each. */
int cpecan_hip_batch_fetch_pairs(cpecan_batch *batch, int64_t item, int64_t *triples, double *logp,
                                 int64_t cap);
/* totalProbability refreshes of one item: the diagonal and the value, in the order computed. */
int cpecan_hip_batch_fetch_totals(cpecan_batch *batch, int64_t item, int64_t *xay, double *total,
                                  int64_t cap);
/* Expectations (mode EXPECTATIONS): per model id, 9 transitions [from*3+to] + 4096 k-mer gap bins
 * + likelihood = 4106 doubles, summed over the items of the batch that use that model. The device
 * buffer pointer is exposed so that a caller can all-reduce it in place (RCCL) before fetching. */
#define CPECAN_EXPECTATION_LEN (9 + CPECAN_NUM_KMERS + 1)
/* DNA batches (HmmDiscrete, impl/discreteHmm.c:10-153): 25 transitions [from*5+to], 5 x 16 emissions
 * [state*16 + x*4 + y] (cell_updateExpectations :407-424) + likelihood, per cpecan_hip_models5_create id */
#define CPECAN_EXPECTATION5_LEN (25 + 5 * 16 + 1)
/* vanilla batches (VanillaHmm, impl/continuousHmm.c:373-466): skip bins 0..29 beta (match -> gapX), 30..59
 * alpha (gapX -> gapX) (cell_signal_updateBetaAndAlphaProb :478-498) + likelihood, per modelsv_create id */
#define CPECAN_EXPECTATIONV_LEN (60 + 1)
/* HDP batches (HdpHmm, impl/continuousHmm.c:631-697): 9 transitions [from*3+to] + likelihood per
 * cpecan_hip_modelsh_create id; params->threshold is the HdpHmm's assignment threshold, and the event-to-k-mer
 * assignments of an item (cell_signal_updateTransAndKmerSkipExpectations2 impl/pairwiseAligner.c:445-476) come
 * back through cpecan_hip_batch_fetch_pairs as (from state, x, y) triples in the reference's order, logp = the
 * transition's log posterior */
#define CPECAN_EXPECTATIONH_LEN (9 + 1)
int cpecan_hip_batch_expectations_device_ptr(cpecan_batch *batch, void **dev_ptr, int64_t *n_doubles);
int cpecan_hip_batch_fetch_expectations(cpecan_batch *batch, int32_t model_id, double *out);
/* The batch's per-model blocks added up on the device: out[i], for the expectation length of the batch's machine (the
 * CPECAN_EXPECTATION*_LEN above), is block 0's value plus block 1's plus ... in ascending model id, in fp64 -- bit for
 * bit the left-to-right host sum of what cpecan_hip_batch_fetch_expectations returns for ids 0 .. n_models - 1 (no
 * reassociation, no tree, no atomics: the order is the contract).  One kernel behind the run's end event, one copy, one
 * wait, however many models the batch has.  The result buffer (that many doubles) is allocated on the batch's account
 * at the first call: CPECAN_ELIMIT where the context's memory limit refuses it, and the call can be made again once
 * there is room.  CPECAN_EINVAL for a batch that was not created for an E-step. */
int cpecan_hip_batch_sum_expectations(cpecan_batch *batch, double *out);
/* Debug: forward cells and backward cells (as they stand when posteriors are taken) of an item,
 * [cell][state] with cells ordered by diagonal then x-y; needs CPECAN_FLAG_DEBUG_DUMP. */
int cpecan_hip_batch_debug_cells(cpecan_batch *batch, int64_t item, double *forward,
                                 double *backward, int64_t n_cells);
int cpecan_hip_batch_destroy(cpecan_batch *batch);

/* Self-test of the systolic kernel's division: evaluates (x - mu) / sigma for n pseudo-random operand
 * triples (event-like x, model-like mu and sigma, derived from seed) both as an IEEE division and as
 * the Markstein-corrected multiply by RN(1/sigma) the kernel uses; *mismatches receives the number
 * of operands where the two doubles differ (expected: 0). */
int cpecan_hip_selftest_division(cpecan_ctx *ctx, int64_t n, uint64_t seed, int64_t *mismatches);

/* Device and pinned host memory released by batches and model tables is kept by the library for the next request
 * (hipMalloc / hipFree wait for the device; up to half of the card's memory by default, CPECAN_ALLOC_CACHE_GB /
 * CPECAN_PINNED_CACHE_GB).  This gives all of it back to the runtime: call it between phases when something else in the
 * process, or on the card, needs the memory. */
int cpecan_hip_trim_cache(void);
/* How many bytes of released device blocks the library keeps at the most (CPECAN_ALLOC_CACHE_GB, or half of the memory
 * of the card the context is on).  This bounds the blocks nobody holds; a context's memory limit bounds the ones it
 * holds: the two are separate. */
int cpecan_hip_cache_capacity(cpecan_ctx *ctx, int64_t *device_bytes);

/* Stream of the context as an opaque pointer (a hipStream_t) for callers' own work (e.g. an RCCL all-reduce of the
 * expectations): the forward stream of the context's lane set (cpecan_hip_batch_run_after).  A run of a wave batch
 * of one stream group ends on the lane set's post stream, not on this one (other runs -- workgroup kernels, several
 * stream groups, the general kernels -- do end on it), and the stream may carry other contexts' runs: work that needs
 * a batch's results goes after cpecan_hip_batch_sync. */
int cpecan_hip_ctx_stream(cpecan_ctx *ctx, void **stream);

#ifdef __cplusplus
}
#endif
#endif
