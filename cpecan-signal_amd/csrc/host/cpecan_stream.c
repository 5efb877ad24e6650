/*
 * cpecan_stream.c -- the stream of include/cpecan_api.h: reads one at a time, grouped by the kernel each would run on
 * alone, cut into chunks that fit a device-memory budget, the chunks chained on the device while host threads prepare
 * the next and finish the previous one.  A chunk is a Run of cpecan_api.c and goes through run_reads' own steps; what
 * is here is the order of things: the groups (cpecan_stream_plan.c), the slots, the producers' turns, the consumer.
 *
 * The life of a chunk:
 *   closed    (submit / flush)  waits in `pending`, in closing order, until a slot is free and a producer takes it --
 *                               slot and turn are taken together, so whoever holds a turn can prepare
 *   prepared  (a producer)      size_inputs, dedupe_models, pack_reads, create_batch on the slot's context
 *   queued    (that producer)   when its turn has come: cpecan_hip_batch_run_after behind the run queued before it
 *   finished  (the consumer)    sync, collect_pairs, onResult per read, batch destroyed, slot freed -- a stream opened
 *                               for expectations: sync, collect_expectations into temporaries, batch destroyed, the
 *                               temporaries added to the caller's struct, onDone per read
 * CPECAN_ELIMIT from any of these calls cuts the chunk in half; the first half goes on in the chunk's place (a producer
 * keeps slot and turn), the second goes to the head of `pending`.
 */
#include "cpecan_host_private.h"
#include "cpecan_band_extent.h"

#include <pthread.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <time.h>

#define die cpecan_die
/* any failure but the memory limit's ends the process, as everywhere in this library */
#define CHECK(call)                                                                              \
    do {                                                                                         \
        int rc_ = (call);                                                                        \
        if (rc_ != CPECAN_OK) die("cpecan: %s failed (%d): %s", #call, rc_, cpecan_hip_last_error()); \
    } while (0)

/* CPECAN_TIMING=1: where a stream's wall clock goes, on stderr as the C-ABI's own laps -- per chunk what its producer and
 * the consumer spent in each step, at close what the submitting thread spent packing and waiting */
static double now_ms(void) {
    struct timespec t;
    clock_gettime(CLOCK_MONOTONIC, &t);
    return (double) t.tv_sec * 1e3 + (double) t.tv_nsec * 1e-6;
}

#define PRIOR_BYTES_PER_CELL 64.0 /* what a class's first chunk is sized with (cpecan_api.h) */

typedef struct {
    int64_t tag, cells;
    StreamClass cls;
    StateMachine *sM;
    Run one;          /* the read packed alone: its characters and events are the stream's copy of them */
    Sequence sX, sY;  /* over that copy */
    stList *anchors;  /* copy */
    void *record;     /* row->fill at submission */
} SRead;

typedef struct Chunk {
    struct Chunk *next;
    SRead **reads;
    int64_t n;
    int32_t halvings;
    /* from the moment a producer takes it */
    int slot;
    int64_t turn;
    Run run;
    StateMachine **sMs;
    Sequence **sXs, **sYs;
    stList **anchorLists;
    void *records;
    cpecan_batch *batch;
    bool refused; /* one read, and the limit still said no */
} Chunk;

typedef struct {
    StreamClass cls;
    double bytesPerCell;
} ClassStat;

struct cpecan_stream {
    PairwiseAlignmentParameters p;
    bool raggedL, raggedR;
    cpecan_stream_options o;
    cpecan_stream_result_fn onResult;
    cpecan_stream_done_fn onDone; /* (expectations) */
    cpecan_stream_chunk_fn onChunk;
    void *arg;
    int mode;                     /* 0: posterior decode, lists to onResult; 1: the E-step, sums into `expectations` */
    void *expectations;           /* what Run.hmmOut is for the machine of the first read */
    int32_t reqKernel[HM_COUNT], reqFlags[HM_COUNT]; /* what a batch of each machine is asked for, taken at open
                                                        (posterior_request / expectations_request) */
    const MachineRow *row; /* the machine of the first read */
    StreamPlanner planner; /* (the submitting thread's) */
    int64_t perSlot;       /* deviceBytes / slots */
    bool timing;           /* CPECAN_TIMING */
    double msOpen, msPack, msBlocked; /* (the submitting thread's) */

    pthread_mutex_t mu;    /* everything below */
    pthread_cond_t cv;     /* any change of it */
    Chunk *pending, *pendingTail; /* closed, not taken */
    Chunk *queued, *queuedTail;   /* run queued (or refused), in turn order, for the consumer */
    cpecan_ctx **ctx;
    bool *slotBusy;
    int64_t alive;         /* chunks closed and not finished */
    int64_t nextTurn, turn;
    bool stop;
    ClassStat *stats;
    int64_t nStats;
    int64_t nChunks, nRefused;

    pthread_mutex_t runMu; /* queueing a run behind lastRun, and destroying the batch lastRun names */
    cpecan_batch *lastRun;
    pthread_mutex_t callMu; /* the two callbacks */
    pthread_t *producers, consumer;
};

/* ---- reads ---- */
static void read_free(SRead *rd) {
    run_release(&rd->one);
    stList_destruct(rd->anchors);
    free(rd->record);
    free(rd);
}

/* whether a vanilla read meets a k-mer that is none, by the rule batch creation applies to its items */
static bool meets_no_kmer(const Run *one) {
    for (int64_t k = 0; k < one->nItems; k++)
        if (cpecan_item_meets_no_kmer(one->chars + one->items[k].x_offset, one->items[k].lX)) return true;
    return false;
}

/* the class of a read packed alone, and its size in cells */
static void classify(cpecan_stream *s, SRead *rd) {
    const Run *one = &rd->one;
    int32_t widest = 0, stepByOne = 1;
    rd->cells = 0;
    for (int64_t k = 0; k < one->nItems; k++) {
        const cpecan_item *it = &one->items[k];
        int32_t w = 0, st = 1;
        const int rc = cpecan_band_extent(one->anchors + 2 * it->anchor_offset, it->n_anchors, it->lX, it->lY,
                                          s->p.diagonalExpansion, &w, &st);
        if (rc != CPECAN_OK) die("cpecan: the anchors of read %lld do not describe a valid band (%d)", (long long) rd->tag, rc);
        if (w > widest) widest = w;
        stepByOne = stepByOne && st;
        rd->cells += (it->lX + it->lY + 1) * (int64_t) w;
    }
    const StreamClass general = { CPECAN_KERNEL_GENERAL, 0, 0 }, none = { 0, 0, 0 };
    if (s->o.oneClass) {
        rd->cls = none;
        return;
    }
    const int32_t machine = (int32_t) (s->row - MACHINES);
    if (machine == HM_VANILLA && meets_no_kmer(one)) { /* (the choice's one input that is not a number of the band) */
        rd->cls = general;
        return;
    }
    CHECK(cpecan_hip_plan_dispatch(machine, s->mode ? CPECAN_MODE_EXPECTATIONS : CPECAN_MODE_POSTERIOR, s->reqKernel[machine],
                                   s->reqFlags[machine], widest, stepByOne, &rd->cls.kernel, &rd->cls.wave, &rd->cls.rows,
                                   NULL));
}

/* ---- chunks ---- */
static Chunk *chunk_new(SRead **reads, int64_t n, int32_t halvings) {
    Chunk *c = calloc(1, sizeof *c);
    c->reads = reads;
    c->n = n;
    c->halvings = halvings;
    c->slot = -1;
    return c;
}

static void chunk_release_run(Chunk *c) {
    run_release(&c->run);
    memset(&c->run, 0, sizeof c->run);
    free(c->sMs); free(c->sXs); free(c->sYs); free(c->anchorLists); free(c->records);
    c->sMs = NULL; c->sXs = c->sYs = NULL; c->anchorLists = NULL; c->records = NULL;
}

static void chunk_free(Chunk *c) {
    chunk_release_run(c);
    for (int64_t i = 0; i < c->n; i++) read_free(c->reads[i]);
    free(c->reads);
    free(c);
}

/* the second half leaves as a chunk of its own; the first stays in c */
static Chunk *chunk_halve(Chunk *c) {
    const int64_t keep = (c->n + 1) / 2, rest = c->n - keep;
    SRead **second = malloc(sizeof(SRead *) * (size_t) rest);
    memcpy(second, c->reads + keep, sizeof(SRead *) * (size_t) rest);
    c->n = keep;
    c->halvings++;
    return chunk_new(second, rest, c->halvings);
}

static void destroy_batch(cpecan_stream *s, Chunk *c) {
    if (!c->batch) return;
    pthread_mutex_lock(&s->runMu); /* (no run is being queued behind it at this moment) */
    if (s->lastRun == c->batch) s->lastRun = NULL;
    CHECK(cpecan_hip_batch_destroy(c->batch));
    pthread_mutex_unlock(&s->runMu);
    c->batch = NULL;
}

/* models, then the batch, on the slot's context; CPECAN_ELIMIT: nothing of it is left on the device */
static int chunk_prepare(cpecan_stream *s, Chunk *c) {
    cpecan_ctx *ctx = s->ctx[c->slot];
    const size_t n = (size_t) c->n, size = s->row->modelSize;
    c->sMs = malloc(sizeof(StateMachine *) * n);
    c->sXs = malloc(sizeof(Sequence *) * n);
    c->sYs = malloc(sizeof(Sequence *) * n);
    c->anchorLists = malloc(sizeof(stList *) * n);
    c->records = malloc(size * n);
    for (size_t i = 0; i < n; i++) {
        SRead *rd = c->reads[i];
        c->sMs[i] = rd->sM;
        c->sXs[i] = &rd->sX;
        c->sYs[i] = &rd->sY;
        c->anchorLists[i] = rd->anchors;
        memcpy((char *) c->records + size * i, rd->record, size);
    }
    const Run r = { .n = c->n, .sMs = c->sMs, .sXs = c->sXs, .sYs = c->sYs, .anchorLists = c->anchorLists, .p = &s->p,
                    .raggedL = s->raggedL, .raggedR = s->raggedR, .records = c->records, .mode = s->mode,
                    .hmmOut = s->expectations, .requestFlags = &s->reqFlags[s->row - MACHINES] };
    c->run = r;
    const double t0 = now_ms();
    size_inputs(&c->run);
    int rc = dedupe_models(&c->run, ctx);
    const double t1 = now_ms();
    double t2 = t1;
    if (rc == CPECAN_OK) {
        pack_reads(&c->run);
        t2 = now_ms();
        if (c->run.nItems > 0) rc = create_batch(&c->run, ctx, &c->batch);
    }
    if (s->timing)
        fprintf(stderr, "[cpecan timing] stream chunk %lld (%lld reads, slot %d): models %.1f ms, pack %.1f ms, batch %.1f ms\n",
                (long long) c->turn, (long long) c->n, c->slot, t1 - t0, t2 - t1, now_ms() - t2);
    if (rc != CPECAN_OK) {
        if (rc != CPECAN_ELIMIT) die("cpecan: preparing a chunk of the stream failed (%d): %s", rc, cpecan_hip_last_error());
        CHECK(cpecan_hip_models_clear(ctx)); /* (whatever tables there were go back, for the half that follows) */
        chunk_release_run(c);
    }
    return rc;
}

static void report_chunk(cpecan_stream *s, Chunk *c) {
    cpecan_stream_chunk info = { .index = c->turn, .nReads = c->n, .nItems = c->run.nItems, .halvings = c->halvings };
    CHECK(cpecan_hip_ctx_memory(s->ctx[c->slot], &info.deviceBytes, NULL, 0));
    if (c->batch) {
        CHECK(cpecan_hip_batch_info(c->batch, &info.kernel, NULL, &info.maxWidth));
        if (info.kernel == CPECAN_KERNEL_SYSTOLIC) {
            CHECK(cpecan_hip_batch_kernel_family(c->batch, &info.wave));
            CHECK(cpecan_hip_batch_systolic_rows(c->batch, &info.rows));
        } else if (s->row == &MACHINES[HM_DNA5] || s->row == &MACHINES[HM_SM4]) /* (their one-wave kernels) */
            CHECK(cpecan_hip_batch_kernel_family(c->batch, &info.wave));
    }
    /* what a cell of this class costs, for the chunks of the class that close from now on */
    int64_t cells = 0;
    for (int64_t i = 0; i < c->n; i++) cells += c->reads[i]->cells;
    pthread_mutex_lock(&s->mu);
    ClassStat *st = NULL;
    for (int64_t k = 0; k < s->nStats && !st; k++)
        if (memcmp(&s->stats[k].cls, &c->reads[0]->cls, sizeof(StreamClass)) == 0) st = &s->stats[k];
    if (!st) {
        s->stats = realloc(s->stats, sizeof(ClassStat) * (size_t) (s->nStats + 1));
        st = &s->stats[s->nStats++];
        st->cls = c->reads[0]->cls;
        st->bytesPerCell = 0.0;
    }
    if (cells > 0 && (double) info.deviceBytes / (double) cells > st->bytesPerCell)
        st->bytesPerCell = (double) info.deviceBytes / (double) cells;
    s->nChunks++;
    pthread_mutex_unlock(&s->mu);
    if (s->onChunk) {
        pthread_mutex_lock(&s->callMu);
        s->onChunk(s->arg, &info);
        pthread_mutex_unlock(&s->callMu);
    }
}

static void push_pending_front(cpecan_stream *s, Chunk *c) { /* (under mu) */
    c->next = s->pending;
    s->pending = c;
    if (!s->pendingTail) s->pendingTail = c;
    s->alive++;
}

static void *producer_main(void *arg) {
    cpecan_stream *s = arg;
    for (;;) {
        pthread_mutex_lock(&s->mu);
        int slot = -1;
        for (;;) {
            for (int k = 0; k < s->o.slots && slot < 0; k++)
                if (!s->slotBusy[k]) slot = k;
            if ((s->pending && slot >= 0) || s->stop) break;
            slot = -1;
            pthread_cond_wait(&s->cv, &s->mu);
        }
        if (!s->pending || slot < 0) { /* (stop, and nothing left to take) */
            pthread_mutex_unlock(&s->mu);
            return NULL;
        }
        Chunk *c = s->pending;
        s->pending = c->next;
        if (!s->pending) s->pendingTail = NULL;
        c->next = NULL;
        c->slot = slot;
        s->slotBusy[slot] = true;
        c->turn = s->nextTurn++;
        pthread_mutex_unlock(&s->mu);

        bool myTurn = false;
        for (;;) {
            int rc = chunk_prepare(s, c);
            if (rc == CPECAN_OK) {
                const double t0 = now_ms();
                if (!myTurn) {
                    pthread_mutex_lock(&s->mu);
                    while (s->turn != c->turn) pthread_cond_wait(&s->cv, &s->mu);
                    pthread_mutex_unlock(&s->mu);
                    myTurn = true;
                }
                const double t1 = now_ms();
                if (c->batch) {
                    pthread_mutex_lock(&s->runMu);
                    rc = cpecan_hip_batch_run_after(c->batch, s->lastRun);
                    if (rc == CPECAN_OK) s->lastRun = c->batch;
                    pthread_mutex_unlock(&s->runMu);
                    if (s->timing)
                        fprintf(stderr, "[cpecan timing] stream chunk %lld: waited %.1f ms for its turn, run queued in %.1f ms, at %.1f\n",
                                (long long) c->turn, t1 - t0, now_ms() - t1, now_ms());
                    if (rc != CPECAN_OK && rc != CPECAN_ELIMIT)
                        die("cpecan: queueing a chunk of the stream failed (%d): %s", rc, cpecan_hip_last_error());
                }
                if (rc == CPECAN_OK) {
                    report_chunk(s, c);
                    break;
                }
                destroy_batch(s, c);
                CHECK(cpecan_hip_models_clear(s->ctx[c->slot]));
                chunk_release_run(c);
            }
            /* the limit: half the chunk, in the chunk's place; the other half next in line */
            if (c->n == 1) {
                c->refused = true;
                break;
            }
            Chunk *second = chunk_halve(c);
            pthread_mutex_lock(&s->mu);
            push_pending_front(s, second);
            pthread_cond_broadcast(&s->cv);
            pthread_mutex_unlock(&s->mu);
        }
        pthread_mutex_lock(&s->mu);
        while (s->turn != c->turn) pthread_cond_wait(&s->cv, &s->mu);
        if (s->queuedTail) s->queuedTail->next = c;
        else s->queued = c;
        s->queuedTail = c;
        s->turn++;
        pthread_cond_broadcast(&s->cv);
        pthread_mutex_unlock(&s->mu);
    }
}

static void deliver(cpecan_stream *s, int64_t tag, stList *list, bool refused) {
    pthread_mutex_lock(&s->callMu);
    if (!s->mode) s->onResult(s->arg, tag, list);
    else if (s->onDone) s->onDone(s->arg, tag, refused);
    pthread_mutex_unlock(&s->callMu);
}

static void *consumer_main(void *arg) {
    cpecan_stream *s = arg;
    for (;;) {
        pthread_mutex_lock(&s->mu);
        while (!s->queued && !s->stop) pthread_cond_wait(&s->cv, &s->mu);
        Chunk *c = s->queued;
        if (!c) {
            pthread_mutex_unlock(&s->mu);
            return NULL;
        }
        s->queued = c->next;
        if (!s->queued) s->queuedTail = NULL;
        c->next = NULL;
        pthread_mutex_unlock(&s->mu);

        stList **lists = calloc((size_t) c->n, sizeof(stList *));
        ChunkExpectations sums = { NULL, NULL, 0 };
        int rc = CPECAN_OK;
        const double t0 = now_ms();
        double t1 = t0;
        if (!c->refused) {
            if (c->batch) rc = cpecan_hip_batch_sync(c->batch);
            t1 = now_ms();
            if (rc == CPECAN_OK) rc = s->mode ? collect_expectations(&c->run, c->batch, &sums) : collect_pairs(&c->run, c->batch, lists);
            if (rc != CPECAN_OK && rc != CPECAN_ELIMIT)
                die("cpecan: reading a chunk of the stream back failed (%d): %s", rc, cpecan_hip_last_error());
        }
        const double t2 = now_ms();
        destroy_batch(s, c);
        const double t3 = now_ms();
        Chunk *halves[2] = { NULL, NULL };
        if (rc == CPECAN_ELIMIT && c->n > 1) { /* the readback's buffers did not fit: both halves go round again */
            chunk_release_run(c);
            halves[1] = chunk_halve(c);
            halves[0] = chunk_new(c->reads, c->n, c->halvings);
            c->reads = NULL;
            c->n = 0;
        } else {
            /* the whole readback of the chunk has succeeded: only now does the caller's struct change, chunk after chunk
             * in turn order (a chunk that was halved above has added nothing) */
            const bool refused = c->refused || rc != CPECAN_OK;
            if (s->mode && !refused) {
                int64_t *tags = malloc(sizeof(int64_t) * (size_t) c->n);
                for (int64_t i = 0; i < c->n; i++) tags[i] = c->reads[i]->tag;
                apply_expectations(&c->run, &sums, tags);
                free(tags);
            }
            for (int64_t i = 0; i < c->n; i++) deliver(s, c->reads[i]->tag, refused ? NULL : lists[i], refused);
        }
        chunk_expectations_release(&sums);
        free(lists);
        if (s->timing)
            fprintf(stderr, "[cpecan timing] stream chunk %lld: sync %.1f ms, %s %.1f ms, batch destroyed in %.1f ms, results delivered in %.1f ms, at %.1f\n",
                    (long long) c->turn, t1 - t0, s->mode ? "expectations" : "pairs", t2 - t1, t3 - t2, now_ms() - t3, now_ms());
        pthread_mutex_lock(&s->mu);
        if (c->n > 0 && (c->refused || rc != CPECAN_OK)) s->nRefused += c->n;
        if (halves[0]) {
            push_pending_front(s, halves[1]);
            push_pending_front(s, halves[0]);
        }
        s->slotBusy[c->slot] = false;
        s->alive--;
        pthread_cond_broadcast(&s->cv);
        pthread_mutex_unlock(&s->mu);
        chunk_free(c);
    }
}

/* ---- the caller's side ---- */
/* a closed group becomes a chunk; waits while `slots` chunks are alive */
static void enqueue(cpecan_stream *s, StreamGroup *g) {
    Chunk *c = chunk_new((SRead **) g->items, g->n, 0);
    const double t0 = now_ms();
    pthread_mutex_lock(&s->mu);
    while (s->alive >= s->o.slots) pthread_cond_wait(&s->cv, &s->mu);
    s->msBlocked += now_ms() - t0;
    if (s->pendingTail) s->pendingTail->next = c;
    else s->pending = c;
    s->pendingTail = c;
    s->alive++;
    pthread_cond_broadcast(&s->cv);
    pthread_mutex_unlock(&s->mu);
}

/* mode 0: onResult; mode 1: expectations, onDone (which may be NULL) */
static cpecan_stream *stream_open(PairwiseAlignmentParameters *p, bool raggedL, bool raggedR, const cpecan_stream_options *o,
                                  int mode, cpecan_stream_result_fn onResult, void *expectations, cpecan_stream_done_fn onDone,
                                  cpecan_stream_chunk_fn onChunk, void *arg) {
    cpecan_stream *s = calloc(1, sizeof *s);
    const double t0 = now_ms();
    s->timing = getenv("CPECAN_TIMING") != NULL;
    s->p = *p;
    s->raggedL = raggedL;
    s->raggedR = raggedR;
    if (o) s->o = *o;
    if (s->o.slots == 0) s->o.slots = 4;
    if (s->o.producerThreads == 0) s->o.producerThreads = 2;
    if (s->o.maxReadsPerChunk == 0) s->o.maxReadsPerChunk = 1024;
    if (s->o.slots < 2 || s->o.producerThreads < 1 || s->o.maxReadsPerChunk < 1 || s->o.deviceBytes < 0)
        die("cpecan_stream_open: at least 2 slots, 1 producer thread and 1 read per chunk, and no negative budget");
    s->onResult = onResult;
    s->onDone = onDone;
    s->onChunk = onChunk;
    s->arg = arg;
    s->mode = mode;
    s->expectations = expectations;
    for (int m = 0; m < HM_COUNT; m++) { /* (an E-step's: with the environment's switches as they stand now) */
        if (mode) expectations_request(&MACHINES[m], &s->reqKernel[m], &s->reqFlags[m]);
        else posterior_request(&MACHINES[m], &s->reqKernel[m], &s->reqFlags[m]);
    }
    planner_init(&s->planner, s->o.maxReadsPerChunk);
    pthread_mutex_init(&s->mu, NULL);
    pthread_mutex_init(&s->runMu, NULL);
    pthread_mutex_init(&s->callMu, NULL);
    pthread_cond_init(&s->cv, NULL);
    s->ctx = calloc((size_t) s->o.slots, sizeof(cpecan_ctx *));
    s->slotBusy = calloc((size_t) s->o.slots, sizeof(bool));
    const char *dev = getenv("CPECAN_DEVICE");
    for (int k = 0; k < s->o.slots; k++) CHECK(cpecan_hip_ctx_create(dev ? atoi(dev) : 0, &s->ctx[k]));
    if (s->o.deviceBytes == 0) CHECK(cpecan_hip_cache_capacity(s->ctx[0], &s->o.deviceBytes));
    s->perSlot = s->o.deviceBytes / s->o.slots;
    if (s->perSlot < 1) s->perSlot = 1;
    for (int k = 0; k < s->o.slots; k++) CHECK(cpecan_hip_ctx_set_memory_limit(s->ctx[k], s->perSlot));
    s->producers = calloc((size_t) s->o.producerThreads, sizeof(pthread_t));
    for (int k = 0; k < s->o.producerThreads; k++)
        if (pthread_create(&s->producers[k], NULL, producer_main, s) != 0) die("cpecan_stream_open: cannot start a thread");
    if (pthread_create(&s->consumer, NULL, consumer_main, s) != 0) die("cpecan_stream_open: cannot start a thread");
    s->msOpen = now_ms() - t0;
    return s;
}

cpecan_stream *cpecan_stream_open(PairwiseAlignmentParameters *p, bool raggedL, bool raggedR, const cpecan_stream_options *o,
                                  cpecan_stream_result_fn onResult, cpecan_stream_chunk_fn onChunk, void *arg) {
    if (!p || !onResult) die("cpecan_stream_open: parameters and a result callback are needed");
    return stream_open(p, raggedL, raggedR, o, 0, onResult, NULL, NULL, onChunk, arg);
}

cpecan_stream *cpecan_stream_open_expectations(PairwiseAlignmentParameters *p, bool raggedL, bool raggedR,
                                               const cpecan_stream_options *o, void *expectations,
                                               cpecan_stream_done_fn onDone, cpecan_stream_chunk_fn onChunk, void *arg) {
    if (!p || !expectations) die("cpecan_stream_open_expectations: parameters and the struct the expectations go to are needed");
    return stream_open(p, raggedL, raggedR, o, 1, NULL, expectations, onDone, onChunk, arg);
}

/* Test hook: the class of an E-step read of the machine whose widest band is maxWidth, as classify takes it */
int32_t cpecan_stream_expectations_class(int32_t machine, int32_t maxWidth, int32_t edgesStepByOne, int32_t *kernel,
                                         int32_t *wave, int32_t *rows) {
    if (machine < 0 || machine >= HM_COUNT) return CPECAN_EINVAL;
    int32_t k, f;
    expectations_request(&MACHINES[machine], &k, &f);
    return cpecan_hip_plan_dispatch(machine, CPECAN_MODE_EXPECTATIONS, k, f, maxWidth, edgesStepByOne, kernel, wave, rows, NULL);
}

void cpecan_stream_submit(cpecan_stream *s, int64_t tag, StateMachine *sM, Sequence *sX, Sequence *sY, stList *anchors) {
    const double t0 = now_ms();
    const HostMachine kind = check_known_combination(sM, sX, sY);
    if (!s->row) s->row = &MACHINES[kind];
    if (s->row != &MACHINES[kind]) die("cpecan: one call cannot mix state machine kinds");
    SRead *rd = calloc(1, sizeof *rd);
    rd->tag = tag;
    rd->sM = sM;
    rd->record = calloc(1, s->row->modelSize);
    s->row->fill(sM, rd->record);
    rd->anchors = stList_construct3(0, (void (*)(void *)) stIntTuple_destruct);
    for (int64_t k = 0; anchors && k < stList_length(anchors); k++) {
        stIntTuple *t = stList_get(anchors, k);
        stList_append(rd->anchors, stIntTuple_construct2(stIntTuple_get(t, 0), stIntTuple_get(t, 1)));
    }
    /* the read packed alone, by the steps that pack a chunk: its sub-alignments with their anchors, which its class is
     * taken from, and the copy of its characters and events (no device model yet: id 0 stands in) */
    const Run one = { .n = 1, .sMs = &rd->sM, .sXs = &sX, .sYs = &sY, .anchorLists = &rd->anchors, .p = &s->p,
                      .raggedL = s->raggedL, .raggedR = s->raggedR, .mode = s->mode /* (size_inputs refuses an E-step of a
                                                                                         machine that has none) */ };
    rd->one = one;
    size_inputs(&rd->one);
    rd->one.modelOf = calloc(1, sizeof(int32_t));
    rd->one.ids = calloc(1, sizeof(int32_t));
    pack_reads(&rd->one);
    rd->sX = *sX;
    rd->sX.elements = rd->one.chars;
    rd->sY = *sY;
    rd->sY.elements = s->row->yChars ? (void *) rd->one.ychars : (void *) rd->one.events;
    rd->one.sMs = NULL; /* (the caller's sequences are not looked at again) */
    rd->one.sXs = rd->one.sYs = NULL;
    rd->one.anchorLists = NULL;
    classify(s, rd);

    pthread_mutex_lock(&s->mu);
    double bytesPerCell = PRIOR_BYTES_PER_CELL;
    for (int64_t k = 0; k < s->nStats; k++)
        if (memcmp(&s->stats[k].cls, &rd->cls, sizeof(StreamClass)) == 0 && s->stats[k].bytesPerCell > 0.0)
            bytesPerCell = s->stats[k].bytesPerCell;
    pthread_mutex_unlock(&s->mu);
    s->msPack += now_ms() - t0;
    StreamGroup closed;
    if (planner_add(&s->planner, rd->cls, rd->cells, (int64_t) ((double) s->perSlot / bytesPerCell), rd, &closed))
        enqueue(s, &closed);
}

void cpecan_stream_flush(cpecan_stream *s) {
    StreamGroup closed;
    while (planner_flush_one(&s->planner, &closed)) enqueue(s, &closed);
    pthread_mutex_lock(&s->mu);
    while (s->alive > 0) pthread_cond_wait(&s->cv, &s->mu);
    pthread_mutex_unlock(&s->mu);
}

void cpecan_stream_close(cpecan_stream *s, int64_t *nChunks, int64_t *nRefused, int64_t *peakDeviceBytes) {
    const double t0 = now_ms();
    cpecan_stream_flush(s);
    const double t1 = now_ms();
    pthread_mutex_lock(&s->mu);
    s->stop = true;
    pthread_cond_broadcast(&s->cv);
    pthread_mutex_unlock(&s->mu);
    for (int k = 0; k < s->o.producerThreads; k++) pthread_join(s->producers[k], NULL);
    pthread_join(s->consumer, NULL);
    int64_t peak = 0;
    for (int k = 0; k < s->o.slots; k++) {
        int64_t own = 0;
        CHECK(cpecan_hip_ctx_memory(s->ctx[k], NULL, &own, 0));
        peak += own;
        CHECK(cpecan_hip_ctx_destroy(s->ctx[k]));
    }
    if (s->timing)
        fprintf(stderr, "[cpecan timing] stream: open %.1f ms; submit: packing and classing %.1f ms, blocked on the slots %.1f ms; "
                "close: flush %.1f ms, threads and contexts %.1f ms\n", s->msOpen, s->msPack, s->msBlocked, t1 - t0, now_ms() - t1);
    if (nChunks) *nChunks = s->nChunks;
    if (nRefused) *nRefused = s->nRefused;
    if (peakDeviceBytes) *peakDeviceBytes = peak;
    planner_free(&s->planner);
    pthread_mutex_destroy(&s->mu);
    pthread_mutex_destroy(&s->runMu);
    pthread_mutex_destroy(&s->callMu);
    pthread_cond_destroy(&s->cv);
    free(s->ctx); free(s->slotBusy); free(s->stats); free(s->producers);
    free(s);
}
