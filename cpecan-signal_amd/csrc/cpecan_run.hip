/*
 * cpecan_run.hip -- how a run of a batch is queued: the lanes a chain of batches runs on, the launchers of the three
 * kinds of kernels (the 5-state and 4-state wave kernels, the general kernels, the throughput kernels' sweeps with their event
 * schedule), cpecan_hip_batch_run / _run_after and what a caller asks of a run afterwards (its end, its times, the
 * sweeps' clock).  Which kernels the batch runs on was settled when it was created (choose_dispatch, cpecan_hip.hip);
 * what a finished run gives back: cpecan_readback.hip.  Host code: it defines no kernel.
 */
#include "cpecan_batch.h"

#include "cpecan_sweep.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <new>

extern "C" __global__ void cpecan_k_generale(DevGeneralArgs, DevParams, DevEchelonArgs);
extern "C" __global__ void cpecan_k_wave4_l1(DevGeneralArgs, DevParams);
extern "C" __global__ void cpecan_k_wave4_l2(DevGeneralArgs, DevParams);
#define W5_DECLARE(L)                                                                                             \
    extern "C" __global__ void cpecan_k_wave5_l##L(const DevItem *, DevParams, const int *, const int *,          \
                                                   const long long *, const char *, const char *, const double *, \
                                                   double *, long long *, double *, long long *, long long *,     \
                                                   double *, long long *, double *);                              \
    extern "C" __global__ void cpecan_k_wave5e_l##L(const DevItem *, DevParams, const int *, const int *,         \
                                                    const long long *, const char *, const char *, const double *, \
                                                    double *, long long *, double *, long long *, long long *,    \
                                                    double *, long long *, double *);                             \
    extern "C" __global__ void cpecan_k_wave5p_l##L(const DevItem *, DevParams, const int *, const int *,         \
                                                    const long long *, const char *, const char *, const double *, \
                                                    double *, long long *, double *, long long *, long long *,    \
                                                    double *, long long *, double *);                             \
    extern "C" __global__ void cpecan_k_wave5pe_l##L(const DevItem *, DevParams, const int *, const int *,        \
                                                     const long long *, const char *, const char *, const double *, \
                                                     double *, long long *, double *, long long *, long long *,   \
                                                     double *, long long *, double *);
W5_DECLARE(1)
W5_DECLARE(2)
W5_DECLARE(3)

void lanes_release(LaneSet *L) {
    if (!L || --L->refs > 0) return;
    (void) hipSetDevice(L->device);
    for (hipStream_t s : { L->fwd, L->back, L->post })
        if (s) {
            (void) hipStreamSynchronize(s);
            (void) hipStreamDestroy(s);
        }
    delete L;
}

hipError_t lanes_create(int device, LaneSet **out) {
    *out = nullptr;
    LaneSet *L = new (std::nothrow) LaneSet();
    if (!L) return hipErrorOutOfMemory;
    L->device = device;
    const hipError_t e = hipStreamCreateWithFlags(&L->fwd, hipStreamNonBlocking);
    if (e != hipSuccess) {
        lanes_release(L);
        return e;
    }
    *out = L;
    return hipSuccess;
}

/* the back and post lanes, made when a batch that runs on them is created */
hipError_t lanes_sweeps(LaneSet *L) {
    std::lock_guard<std::mutex> hold(L->mu);
    hipError_t e = hipSuccess;
    for (hipStream_t *s : { &L->back, &L->post })
        if (e == hipSuccess && !*s) e = hipStreamCreateWithFlags(s, hipStreamNonBlocking);
    return e;
}

#define CP_WAVE5_PAIRED_BELOW 1536 /* alignments: below this (fewer than 1.5 per SIMD) the 5-state machine runs on two waves
                                    * per alignment: 1.14-1.24x at 1024 alignments, 0.8-0.9x at 4096 */

/* The 5-state machine for bands a wave covers in one to three cells per lane: one wave per alignment, the recurrence in
 * registers (cpecan_kernel_wave5.hip), posterior decode or expectations */
static int enqueue_wave5(cpecan_batch *b, hipStream_t st) {
    cpecan_ctx *c = b->ctx;
    const bool em = b->mode == CPECAN_MODE_EXPECTATIONS;
    /* a batch that leaves SIMDs with fewer than two waves runs the sweeps of an alignment on a pair of waves
     * (forward and back overlapping); CPECAN_WAVE5_PAIRED=0/1 forces either form (tests, timing) */
    const char *pairedEnv = getenv("CPECAN_WAVE5_PAIRED");
    const int l5 = b->maxWidth <= 64 ? 0 : b->maxWidth <= 128 ? 1 : 2;
    /* (the one-wave E-step at three cells per lane needs more registers than two waves of a SIMD can have) */
    const bool paired = pairedEnv ? atoi(pairedEnv) != 0 : (b->nItems < CP_WAVE5_PAIRED_BELOW || (em && l5 == 2));
    static const auto kernels5 = std::array<decltype(&cpecan_k_wave5_l1), 12>{
        cpecan_k_wave5_l1, cpecan_k_wave5_l2, cpecan_k_wave5_l3, cpecan_k_wave5e_l1, cpecan_k_wave5e_l2, cpecan_k_wave5e_l3,
        cpecan_k_wave5p_l1, cpecan_k_wave5p_l2, cpecan_k_wave5p_l3, cpecan_k_wave5pe_l1, cpecan_k_wave5pe_l2, cpecan_k_wave5pe_l3 };
    auto kernel5 = kernels5[(size_t) ((paired ? 6 : 0) + (em ? 3 : 0) + l5)];
    hipLaunchKernelGGL(kernel5, dim3((unsigned) b->nItems), dim3(paired ? 128 : 64), 0, st, (const DevItem *) b->items.p, b->P,
                       (const int *) b->bandL.p, (const int *) b->bandR.p, (const long long *) b->cellPrefix.p,
                       (const char *) b->chars.p, (const char *) b->charsY.p, (const double *) c->tables[DNA5].block.p,
                       b->Fstore.p, b->pairs.p, b->pairLogp.p, b->nPairs.p, b->totXay.p, b->totVal.p, b->nTot.p,
                       em ? b->expect.p : nullptr);
    HIP_TRY(hipGetLastError());
    return CPECAN_OK;
}

/* what the general kernels are handed, filled from the machine's row */
static DevGeneralArgs general_args(const cpecan_batch *b) {
    const cpecan_ctx *c = b->ctx;
    const MachineRow &m = MACHINES[b->machine];
    const bool em = b->mode == CPECAN_MODE_EXPECTATIONS;
    const void *x = m.x == X_CHARS ? (const void *) b->chars.p : m.x == X_KID ? (const void *) b->kid.p : (const void *) b->kidx.p;
    const void *y = m.x == X_CHARS ? (const void *) b->charsY.p : (const void *) b->events.p; /* (nucleotides on both sides) */
    return { (const DevItem *) b->items.p, (const int *) b->bandL.p, (const int *) b->bandR.p,
             (const long long *) b->cellPrefix.p, x, y, m.yAux ? (const double *) b->logNoise.p : nullptr,
             c->tables[b->machine].block.p, b->Fstore.p, b->Bstore.p, b->pairs.p, b->pairLogp.p, b->nPairs.p, b->totXay.p,
             b->totVal.p, b->nTot.p, b->dbgB.p, em ? b->expect.p : nullptr };
}

/* The 4-state machine for bands a wave covers in one or two cells per lane (CPECAN_FLAG_SM4_WAVE): one wave per
 * alignment, the recurrence in registers (cpecan_kernel_wave4.hip), on the general kernel's buffers */
static int enqueue_wave4(cpecan_batch *b, hipStream_t st) {
    const DevGeneralArgs a = general_args(b);
    hipLaunchKernelGGL(b->maxWidth <= 64 ? cpecan_k_wave4_l1 : cpecan_k_wave4_l2, dim3((unsigned) b->nItems), dim3(64), 0, st, a,
                       b->P);
    HIP_TRY(hipGetLastError());
    return CPECAN_OK;
}

/* The general kernels (cpecan_general.h): one per machine, one parameter list */
static int enqueue_general(cpecan_batch *b, hipStream_t st) {
    const MachineRow &m = MACHINES[b->machine];
    DevGeneralArgs a = general_args(b);
    DevParams P = b->P;
    /* the forward sweep's two previous diagonals live in LDS where the widest band fits (three diagonals of the
     * machine's states: 120 bytes per cell of width for the 5-state machine); CPECAN_GENERAL_LDS=0 keeps them in HBM
     * (timing, tests) */
    static const bool ldsOff = getenv("CPECAN_GENERAL_LDS") != nullptr && atoi(getenv("CPECAN_GENERAL_LDS")) == 0;
    P.ldsWidth = (!ldsOff && b->maxWidth <= m.ldsMaxWidth) ? b->maxWidth : 0;
    const size_t lds = (size_t) P.ldsWidth * 3 * m.states * sizeof(double);
    if (m.general)
        hipLaunchKernelGGL(m.general, dim3((unsigned) b->nItems), dim3(256), lds, st, a, P);
    else { /* (cpecan_kernel_generale.hip) */
        DevEchelonArgs e = { (const char *) b->chars.p, (const long long *) b->xEnd.p, (const double *) b->duration.p };
        hipLaunchKernelGGL(cpecan_k_generale, dim3((unsigned) b->nItems), dim3(256), 0, st, a, P, e);
    }
    HIP_TRY(hipGetLastError());
    return CPECAN_OK;
}

/* the argument record of the sweeps of one run, the models as the sweeps read them */
static SweepArgs sweep_args(const cpecan_batch *b, const ModelTable &table) {
    const SweepBuild *sy = b->sy;
    SweepArgs all{};
    all.items = b->items.p; all.nItems = b->nItems; all.P = b->P; all.bandTab = (const int2 *) b->bandTab.p;
    all.track = b->track.p; all.trackBase = b->trackBase.p; all.maxLX = b->maxLX; all.events = b->events.p;
    all.kidx = b->kidx.p; all.kid = b->kid.p; all.Fring = b->Fstore.p; all.ringDoubles = b->ringDoubles;
    all.ringD = b->ringD; all.states = b->syStates.p; all.stateBytes = b->stateBytes; all.pairs = b->pairs.p;
    all.pairLogp = b->pairLogp.p; all.totXay = b->totXay.p; all.totVal = b->totVal.p; all.scratch = b->syScratch.p;
    all.scratchBytes = b->scratchBytes; all.Bring = b->Bring.p; all.bringRow = sy->bringRowDoubles;
    all.expect = b->expect.p; all.nPairs = b->nPairs.p; all.nTot = b->nTot.p; all.nCells = b->nCells.p;
    /* the models as the sweeps read them, and whether any of them lets gap Y switch to gap X (the nanopore default
     * does not, stateMachine.c:1287: the kernels then run the build without that term; the vanilla machine has no such
     * transition) */
    all.models = table.block.p;
    if (sy->machine == SWEEP_HDP || sy->machine == SWEEP_STRAWMAN)
        for (double switchToX : table.side)
            if (switchToX > -INFINITY) all.withSwitch = 1;
    return all;
}

/* ... and that of the assembly sweeps (the window is set per launch) */
static AsmArgs asm_args(const cpecan_batch *b, const ModelTable &table) {
    const cpecan_ctx *c = b->ctx;
    AsmArgs asmArgs{};
    asmArgs.items = b->items.p; asmArgs.trackBase = b->trackBase.p; asmArgs.planWin = b->planWin.p;
    asmArgs.planCtl = b->planCtl.p; asmArgs.planOff = b->planOff.p; asmArgs.events = b->events.p;
    asmArgs.models = table.block.p; asmArgs.track = b->track.p; asmArgs.ring = b->Fstore.p;
    asmArgs.ringDoubles = b->ringDoubles; asmArgs.states = b->syStates.p; asmArgs.ctx = b->asmCtx.p;
    asmArgs.ctxBytes = asm_format(b->asmCells).ctxBytes; asmArgs.coef = cpecan_asm_coef(c->device); asmArgs.nItems = (int) b->nItems;
    asmArgs.ringD = b->ringD; asmArgs.maxWindows = b->asmMaxWindows; asmArgs.scratch = b->syScratch.p;
    asmArgs.scratchBytes = b->scratchBytes; asmArgs.logThrSlack = b->P.logThrSlack; asmArgs.modelStride = CP_MODEL_STRIDE;
    asmArgs.maskTab = b->asmMasks.p;
    return asmArgs;
}

/* CPECAN_ASM_TRACE: where everything the assembly sweeps are handed lies */
static void asm_trace(const cpecan_batch *b, const AsmArgs &asmArgs) {
    const ModelTable &table = b->ctx->tables[b->machine];
    auto span = [](const char *what, const void *p, size_t bytes) {
        fprintf(stderr, "[cpecan asm]   %-10s %p .. %p (%zu bytes)\n", what, p, (const char *) p + bytes, bytes);
    };
    span("items", b->items.p, b->items.n * sizeof(DevItem));
    span("trackBase", b->trackBase.p, b->trackBase.n * 8);
    span("planWin", b->planWin.p, b->planWin.n * sizeof(AsmPlanWin));
    span("planCtl", b->planCtl.p, b->planCtl.n * sizeof(AsmPlanCtl));
    span("planOff", b->planOff.p, b->planOff.n * 8);
    span("events", b->events.p, b->events.n * 8);
    span("models", table.block.p, table.block.n * 8);
    span("track", b->track.p, b->track.n * 8);
    span("ring", b->Fstore.p, b->Fstore.n * 8);
    span("states", b->syStates.p, b->syStates.n);
    span("ctx", b->asmCtx.p, b->asmCtx.n);
    span("scratch", b->syScratch.p, b->syScratch.n);
    span("masks", b->asmMasks.p, b->asmMasks.n * 4);
    span("coef", asmArgs.coef, 512);
    fprintf(stderr, "[cpecan asm]   ringD %d ringDoubles %lld windows %d scratchBytes %lld\n", b->ringD, b->ringDoubles,
            b->asmMaxWindows, b->scratchBytes);
}

/* The throughput kernels, one pass: the per-item track of emission constants (a function of the inputs, rebuilt every
 * run inside the timed region), then for every traceback window the forward kernel and the backward kernel.  The wave
 * kernels run the two on streams of their own: the sweep back of window w overlaps the forward sweep of window w+1 of the
 * same alignments (each SIMD then holds a forward and a backward wave), and forward w+2, which re-uses window w's ring
 * rows, waits for the sweep back of w.  Events around every kernel give per-kernel times and carry the dependencies.
 * *sEnd: the stream the run ends on (the post lane where it went over the three lanes: *laneRun). */
static int enqueue_sweeps(cpecan_batch *b, LaneSet *L, hipStream_t *sEnd, bool *laneRun) {
    cpecan_ctx *c = b->ctx;
    const SweepBuild *sy = b->sy;
    const int G = b->nGroups, perGroup = 4 * b->nWindows + 1;
    if (b->evStage.size() != (size_t) (G * perGroup)) {
        for (hipEvent_t e : b->evStage) (void) hipEventDestroy(e);
        b->evStage.assign((size_t) (G * perGroup), nullptr);
        for (auto &e : b->evStage) HIP_TRY(hipEventCreate(&e));
    }
    const ModelTable &table = c->tables[b->machine];
    const SweepArgs all = sweep_args(b, table);
    int rc = sy->once->launch_track(L->fwd, all);
    /* the assembly sweeps (no model of the batch may let gap Y switch to gap X: they have no such term) */
    const bool asmRun = b->useAsm && !all.withSwitch && rc == 0;
    AsmArgs asmArgs{};
    if (asmRun) {
        asmArgs = asm_args(b, table);
        rc = cpecan_asm_launch_begin(L->fwd, b->items.p, b->nItems, b->Fstore.p, b->ringDoubles, b->asmCells);
        if (getenv("CPECAN_ASM_TRACE")) asm_trace(b, asmArgs);
    }
    HIP_TRY(hipEventRecord(b->evFork, L->fwd));
    *laneRun = !b->gStreamOwned;
    if (*laneRun && (!L->back || !L->post)) return fail(CPECAN_EHIP, "lane set without its sweep lanes");
    if (*laneRun) *sEnd = L->post;
#ifdef CPECAN_TIMING_BUILD
    static const bool fwdOnly = getenv("CPECAN_TIMING_FORWARD_ONLY") != nullptr; /* timing study: wrong results */
    static const bool noPost = getenv("CPECAN_TIMING_NO_POST") != nullptr;       /* timing study: sweeps only */
#else
    const bool fwdOnly = false, noPost = false;
#endif
    const long long per = (b->nItems + G - 1) / G;
    for (int gi = 0; gi < G && rc == 0; gi++) {
        const long long i0 = gi * per, n = std::min<long long>(per, b->nItems - i0);
        SweepArgs a = all.slice(i0, n);
        hipStream_t sF = *laneRun ? L->fwd : b->gStream[(size_t) gi];
        hipStream_t sB = *laneRun ? L->back : sy->wave ? b->gStreamB[(size_t) gi] : sF;
#ifdef CPECAN_TIMING_BUILD
        if (getenv("CPECAN_TIMING_SERIAL")) sB = sF; /* timing study: every sweep alone on the chip */
#endif
        hipEvent_t *ev = b->evStage.data() + (size_t) gi * perGroup;
        HIP_TRY(hipStreamWaitEvent(sF, b->evFork, 0));
        if (sB != sF) HIP_TRY(hipStreamWaitEvent(sB, b->evFork, 0));
        HIP_TRY(hipEventRecord(ev[0], sF));
        for (int w = 0; w < b->nWindows && rc == 0; w++) {
            hipEvent_t *e4 = ev + 1 + 4 * w;
            /* assembly sweeps: the window's totals and decode (and the re-sweep of what cannot be trusted) run on a
             * stream of their own.  The sweep back of the next window does not wait for them (it fills the other
             * half of the scratch), nor does the forward sweep of window w+2 (the ring holds three windows, the
             * state four window records); what does: the sweep back of w+2 (scratch), the forward sweep of w+3
             * (ring rows, window record).  The forward sweep of w+2 still waits for the sweep back of w, which reads
             * the context that sweep will overwrite when it ends. */
            const bool postAside = asmRun && b->asmBackward && sB != sF && b->postAside && *laneRun;
            if (postAside) a.scratch = b->syScratch.p + (size_t) (w & 1) * (size_t) b->nItems * (size_t) b->scratchBytes;
            if (sB != sF && w >= 2) HIP_TRY(hipStreamWaitEvent(sF, ev[1 + 4 * (w - 2) + 3], 0));
            if (postAside && w >= 3) HIP_TRY(hipStreamWaitEvent(sF, b->evPost[(size_t) w - 3], 0));
            HIP_TRY(hipEventRecord(e4[0], sF));
            if (n > 0 && asmRun) {
                asmArgs.window = w;
                rc = cpecan_asm_launch_forward(c->device, sF, &asmArgs, b->asmCells);
            } else if (n > 0)
                rc = sy->forward(sF, a, w);
            HIP_TRY(hipEventRecord(e4[1], sF));
            if (sB != sF) HIP_TRY(hipStreamWaitEvent(sB, e4[1], 0));
            HIP_TRY(hipEventRecord(e4[2], sB));
            if (rc == 0 && n > 0 && asmRun && b->asmBackward && !fwdOnly) {
                asmArgs.window = w;
                asmArgs.scratch = a.scratch;
                if (postAside && w >= 2) HIP_TRY(hipStreamWaitEvent(sB, b->evPost[(size_t) w - 2], 0));
                rc = cpecan_asm_launch_backward(c->device, sB, &asmArgs, b->asmCells);
                hipStream_t sP = postAside ? L->post : sB;
                if (postAside) {
                    HIP_TRY(hipEventRecord(e4[3], sB));
                    HIP_TRY(hipStreamWaitEvent(sP, e4[3], 0));
                }
                if (rc == 0 && !noPost) rc = sy->post_asm(sP, a, w);
                if (postAside) HIP_TRY(hipEventRecord(b->evPost[(size_t) w], sP));
            } else if (rc == 0 && n > 0 && !fwdOnly)
                rc = (b->fused ? sy->backward_fx : sy->backward)(sB, a, w);
            if (rc == 0 && n > 0 && b->mode == CPECAN_MODE_EXPECTATIONS && !b->fused) rc = sy->expect(sB, a, w);
            if (!postAside) HIP_TRY(hipEventRecord(e4[3], sB));
        }
        /* the last sweep back follows every forward sweep; the run ends behind it on the post lane (after the last
         * post kernel there), which leaves the forward lane to the next run's first forward sweep */
        HIP_TRY(hipEventRecord(b->evJoin[(size_t) gi], sB));
        HIP_TRY(hipStreamWaitEvent(*sEnd, b->evJoin[(size_t) gi], 0));
    }
    if (rc == 0) rc = sy->once->launch_counts(*sEnd, all);
    if (rc != 0) return fail(CPECAN_EHIP, "throughput kernel launch failed: %s", hipGetErrorString(hipGetLastError()));
    return CPECAN_OK;
}

/* One run of the batch, queued on the lane set L (its mutex held).  A wave batch of one stream group runs over the
 * three lanes and ends on the post lane; every other batch runs on the forward lane (and streams of its own). */
static int batch_enqueue(cpecan_batch *b, cpecan_batch *after, LaneSet *L) {
    /* its own last run first, wherever it went (the ring, state and scratch are the batch's); then the batch it follows,
     * unless stream order on the lanes already puts this run behind it */
    if (b->ran) HIP_TRY(hipStreamWaitEvent(L->fwd, b->ev2, 0));
    if (after && !(after->laneRun && after->runLanes == L)) HIP_TRY(hipStreamWaitEvent(L->fwd, after->ev2, 0));
    hipStream_t sEnd = L->fwd; /* where the run ends: counts, packing, ev2 */
    bool laneRun = false;
    b->countsValid = false;
    int rc;
    HIP_TRY(hipEventRecord(b->ev0, L->fwd));
    if (b->mode == CPECAN_MODE_EXPECTATIONS)
        HIP_TRY(hipMemsetAsync(b->expect.p, 0, b->expect.n * sizeof(double), L->fwd));
    HIP_TRY(hipEventRecord(b->ev1, L->fwd));
    if (b->wave5)
        rc = enqueue_wave5(b, L->fwd);
    else if (b->wave4)
        rc = enqueue_wave4(b, L->fwd);
    else if (b->kernel == CPECAN_KERNEL_GENERAL)
        rc = enqueue_general(b, L->fwd);
    else
        rc = enqueue_sweeps(b, L, &sEnd, &laneRun);
    if (rc != CPECAN_OK) return rc;
    if ((rc = pack_in_run(b, sEnd)) != CPECAN_OK) return rc;
    HIP_TRY(hipEventRecord(b->ev2, sEnd));
    b->ran = true;
    b->laneRun = laneRun;
    return CPECAN_OK;
}

extern "C" {

int cpecan_hip_batch_run(cpecan_batch *b) { return cpecan_hip_batch_run_after(b, nullptr); }

int cpecan_hip_batch_run_after(cpecan_batch *b, cpecan_batch *after) {
    if (!b) return fail(CPECAN_EINVAL, "batch is NULL");
    cpecan_ctx *c = b->ctx;
    if (!c) return fail(CPECAN_EINVAL, "the batch's context has been destroyed");
    if (b->modelEpoch != c->modelEpoch)
        return fail(CPECAN_EINVAL, "cpecan_hip_models_clear was called on the context after this batch was created: "
                    "its model ids are gone");
    if (after && after->device != b->device) return fail(CPECAN_EINVAL, "the two batches live on different devices");
    HIP_TRY(hipSetDevice(c->device));
    MemScope mem(b->mem); /* (the pack buffers of the run) */
    if (!b->pairsLaidOut) { /* a readback's growth of the pair buffer was refused by the memory limit: made now */
        const int rc = lay_out_pairs(b);
        if (rc != CPECAN_OK) return rc;
    }
    if (after == b || (after && !after->ran)) after = nullptr;
    /* behind a wave batch of one stream group, the whole run goes on the lanes that batch ran on: this batch's first
     * forward sweep follows that batch's LAST FORWARD sweep on the forward lane and shares the SIMDs with its last
     * sweep back, as the forward sweep of that batch's own next window would have; its sweeps back and post kernels
     * queue behind that batch's on the other two lanes.  Otherwise on this context's lanes, behind the whole run of
     * `after`. */
    LaneSet *L = (after && after->laneRun && after->runLanes) ? after->runLanes : c->lanes;
    std::lock_guard<std::mutex> hold(L->mu);
    if (b->runLanes != L) {
        L->refs++;
        lanes_release(b->runLanes);
        b->runLanes = L;
    }
    const int rc = batch_enqueue(b, after, L);
    if (rc != CPECAN_OK) {
        /* what was queued of the run is over before the error goes back (sync and destroy wait for its end event,
         * which it never recorded) */
        for (hipStream_t s : { L->fwd, L->back, L->post })
            if (s) (void) hipStreamSynchronize(s);
        if (b->gStreamOwned)
            for (hipStream_t s : b->gStream) (void) hipStreamSynchronize(s);
        for (hipStream_t s : b->gStreamB) (void) hipStreamSynchronize(s);
        b->ran = false;
        b->laneRun = false;
    }
    return rc;
}

int cpecan_hip_batch_stage_ms(cpecan_batch *b, float *msForward, float *msBackward, int32_t *launchesEach) {
    if (!b || !b->ran) return fail(CPECAN_EINVAL, "batch has not run");
    if (b->kernel != CPECAN_KERNEL_SYSTOLIC) return fail(CPECAN_EINVAL, "only the systolic path has stages");
    HIP_TRY(hipSetDevice(b->ctx->device));
    HIP_TRY(hipEventSynchronize(b->ev2));
    float f = 0, k = 0;
    const int perGroup = 4 * b->nWindows + 1;
    for (int gi = 0; gi < b->nGroups; gi++)
        for (int w = 0; w < b->nWindows; w++) {
            const hipEvent_t *ev = b->evStage.data() + (size_t) gi * perGroup + 1 + 4 * w;
            float a = 0, c2 = 0;
            HIP_TRY(hipEventElapsedTime(&a, ev[0], ev[1]));
            HIP_TRY(hipEventElapsedTime(&c2, ev[2], ev[3]));
            f += a;
            k += c2;
        }
    static const bool timeline = getenv("CPECAN_TIMELINE") != nullptr; /* timing study: when every stage began and ended */
    if (timeline) {
        const hipEvent_t *ev = b->evStage.data();
        for (int w = 0; w < b->nWindows; w++) {
            float t[4] = { 0, 0, 0, 0 };
            for (int q = 0; q < 4; q++) (void) hipEventElapsedTime(&t[q], ev[0], ev[1 + 4 * w + q]);
            fprintf(stderr, "[cpecan timeline] window %2d: forward %7.3f .. %7.3f   backward+post %7.3f .. %7.3f\n", w, t[0], t[1],
                    t[2], t[3]);
        }
    }
    if (msForward) *msForward = f;
    if (msBackward) *msBackward = k;
    if (launchesEach) *launchesEach = b->nWindows * b->nGroups;
    return CPECAN_OK;
}

int cpecan_hip_batch_shader_clock_mhz(cpecan_batch *b, double *mhz) {
    if (!b || !mhz) return fail(CPECAN_EINVAL, "bad argument");
    *mhz = 0.0;
    if (!b->ran || b->kernel != CPECAN_KERNEL_SYSTOLIC || !b->sy->wave) return CPECAN_OK; /* not measured on this path */
    HIP_TRY(hipSetDevice(b->ctx->device));
    HIP_TRY(hipEventSynchronize(b->ev2));
    if (cpecan_wave_shader_clock_mhz(b->ctx->prep, b->syStates.p, b->nItems, mhz) != 0)
        return fail(CPECAN_EHIP, "reading the sweeps' clock counters failed");
    return CPECAN_OK;
}

int cpecan_hip_batch_sync(cpecan_batch *b) {
    if (!b) return fail(CPECAN_EINVAL, "batch is NULL");
    HIP_TRY(hipSetDevice(b->device));
    /* its own end event: the lanes it ran on may already carry the next batch's run */
    if (b->ran) HIP_TRY(hipEventSynchronize(b->ev2));
    return CPECAN_OK;
}

int cpecan_hip_batch_elapsed_ms(cpecan_batch *b, float *msTotal, float *msKernel) {
    if (!b || !b->ran) return fail(CPECAN_EINVAL, "batch has not run");
    HIP_TRY(hipSetDevice(b->ctx->device));
    HIP_TRY(hipEventSynchronize(b->ev2));
    float a = 0, k = 0;
    HIP_TRY(hipEventElapsedTime(&a, b->ev0, b->ev2));
    HIP_TRY(hipEventElapsedTime(&k, b->ev1, b->ev2));
    if (msTotal) *msTotal = a;
    if (msKernel) *msKernel = k;
    return CPECAN_OK;
}

} /* extern "C" */
