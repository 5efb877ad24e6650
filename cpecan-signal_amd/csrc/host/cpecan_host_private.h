/* cpecan_host_private.h -- shared by the C files of libcpecan_host.so (not installed) */
#ifndef CPECAN_HOST_PRIVATE_H_
#define CPECAN_HOST_PRIVATE_H_

#include "cpecan_api.h"
#include "cpecan_hip.h"

#include <stddef.h>

void cpecan_die(const char *fmt, ...) __attribute__((noreturn, format(printf, 1, 2)));

/* NanoporeHDP as far as density queries need it (deserialize_nhdp, cpecan_api.c) */
struct _nanopore_hdp {
    char alphabet[32];
    int64_t alphabetSize, kmerLength, numDps, gridLength, nRows;
    double *grid, *y, *slope; /* y, slope: nRows x gridLength */
    int32_t *kmerRow;         /* per k-mer id: row of the nearest observed ancestor (impl/hdp.c:2588-2590) */
};

/* fills the function-pointer members of a freshly built machine (cpecan_internals.c) */
void cpecan_sm3_set_functions(StateMachine3 *s);
void cpecan_sm3hdp_set_functions(StateMachine3_HDP *s);
void cpecan_sm3vanilla_set_functions(StateMachine3Vanilla *s);
void cpecan_sm5_set_functions(StateMachine5 *s);
/* 1 if cellCalculate and the emission plug-ins are the library's own, i.e. the model the device code implements */
int cpecan_sm_functions_known(StateMachine *sM);

/* ---- the six machines of the GPU path and the record one call of run_reads works on (cpecan_api.c); a chunk of the
 * stream (cpecan_stream.c) is such a record and goes through the same steps.  Not exported. ---- */
#pragma GCC visibility push(hidden)

typedef enum { /* in the order of CPECAN_MACHINE_* (cpecan_hip.h) */
    HM_STRAWMAN, HM_DNA5, HM_VANILLA, HM_HDP, HM_SM4, HM_ECHELON, HM_COUNT
} HostMachine;

typedef struct {
    int64_t read, x1, y1;
} ItemOrigin;

/* One call of run_reads: its arguments and every buffer its steps allocate (run_release frees them all) */
typedef struct {
    const struct MachineRow *row;
    int64_t n;
    StateMachine **sMs;
    Sequence **sXs, **sYs;
    stList **anchorLists;
    PairwiseAlignmentParameters *p;
    bool raggedL, raggedR;
    int mode, unbanded;
    void *hmmOut;
    const int32_t *requestFlags; /* the stream: the flags posterior_request / expectations_request gave at open, the ones its
                                    reads were classed with (NULL: ask now) */
    const void *records; /* the stream: n model records of row->modelSize bytes, filled at submission (NULL: fill now) */
    /* dedupe_models: nModels structs of row->modelSize bytes, the state machine each was filled from */
    void *models;
    StateMachine **owner;
    int32_t *modelOf, *ids, nModels;
    /* pack_reads; nAnchorsGiven in the callers' lists, nAnchors packed (those past a read's last cell are left out) */
    char *chars, *ychars;
    double *events;
    int64_t *anchors, *firstItem, nX, nY, nAnchorsGiven, nAnchors, nItems;
    cpecan_item *items;
    ItemOrigin *origin;
} Run;

typedef struct MachineRow {
    /* recognition: StateMachineType(s), stateNumber, element getters of X and Y, what to say of other getters */
    StateMachineType type, type2;
    int64_t stateNumber;
    void *(*getX)(void *, int64_t), *(*getY)(void *, int64_t);
    const char *gettersText;
    /* input geometry: chars a k-mer sequence spans beyond its length; Y as characters instead of events */
    int64_t xPad;
    bool yChars;
    /* modes: what to say of an E-step where add_expectations is NULL; the same for unbanded == 2 */
    const char *refusal;
    bool noSingleBand;
    bool echelonRuns; /* a cell emits runs of pairs: the look-ahead of pack_items, append_diagonals_upwards */
    /* model: size, fill from a state machine, "the same model" (NULL: the same StateMachine), upload */
    size_t modelSize;
    void (*fill)(StateMachine *sM, void *slot);
    bool (*same)(const void *a, const void *b);
    /* (the two create steps return the C-ABI's code: a context with a memory limit may refuse them) */
    int (*models_create)(cpecan_ctx *ctx, const void *models, int32_t nModels, int32_t *ids);
    int (*batch_create)(cpecan_ctx *ctx, const Run *r, const cpecan_band_params *bp, cpecan_batch **batch);
    void (*add_expectations)(const Run *r, cpecan_batch *batch);
    /* the E-step's sums: doubles per model, and one such block added onto the struct Run.hmmOut points to */
    int32_t expectLen;
    void (*add_block)(void *hmmOut, const double *block);
} MachineRow;

extern const MachineRow MACHINES[HM_COUNT];

/* the machine of a read, or no return: anything but the six combinations of the table is not on the GPU path */
HostMachine check_known_combination(StateMachine *sM, Sequence *sX, Sequence *sY);
/* the steps of run_reads, in its order */
void size_inputs(Run *r);
int dedupe_models(Run *r, cpecan_ctx *ctx);
void pack_reads(Run *r);
int create_batch(Run *r, cpecan_ctx *ctx, cpecan_batch **batch);
int collect_pairs(const Run *r, cpecan_batch *batch, stList **lists);
void run_release(Run *r);
/* kernel argument and flags of a posterior batch of the machine and of an E-step batch (the environment's switches for
 * the fused E-steps among them), as its create call passes them: the create calls take them from these two */
void posterior_request(const MachineRow *row, int32_t *kernel, int32_t *flags);
void expectations_request(const MachineRow *row, int32_t *kernel, int32_t *flags);
/* the E-step readback of a chunk of the stream: into temporaries (returns the C-ABI's code and then leaves none), and
 * from them onto r->hmmOut; an HDP assignment of read i carries tags[i] */
typedef struct {
    double *sums;          /* row->expectLen: the batch's models' blocks added on the device (NULL: nothing ran) */
    int64_t *assignments;  /* HDP: nAssignments x (x, y, read of the chunk), in the order expect_hdp walks them */
    int64_t nAssignments;
} ChunkExpectations;
int collect_expectations(const Run *r, cpecan_batch *batch, ChunkExpectations *t);
void apply_expectations(const Run *r, const ChunkExpectations *t, const int64_t *tags);
void chunk_expectations_release(ChunkExpectations *t);

/* ---- the chunking rule of the stream (cpecan_stream_plan.c, which states it) ---- */
typedef struct {
    int32_t kernel, wave, rows; /* as cpecan_hip_plan_dispatch answers for the read alone */
} StreamClass;
typedef struct {
    StreamClass cls;
    void **items; /* in order of arrival */
    int64_t n, cap, cells, opened;
} StreamGroup;
typedef struct {
    StreamGroup *groups; /* one per class met so far */
    int64_t nGroups, capGroups, maxReads, opened;
} StreamPlanner;
void planner_init(StreamPlanner *pl, int64_t maxReads);
/* item joins the open group of cls; true: that group could not take it and was closed first -- *closed is it, and its
 * items array is the caller's to free */
bool planner_add(StreamPlanner *pl, StreamClass cls, int64_t cells, int64_t cellBudget, void *item, StreamGroup *closed);
/* closes the open group that got its first read earliest; false: none is open */
bool planner_flush_one(StreamPlanner *pl, StreamGroup *closed);
void planner_free(StreamPlanner *pl);

#pragma GCC visibility pop

#endif
