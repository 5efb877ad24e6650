/*
 * cpecan_batch.h -- the batch, as the three files that work on it see it: cpecan_hip.hip chooses its kernels, creates and
 * destroys it, cpecan_run.hip queues its runs, cpecan_readback.hip takes a finished run to the caller's counts and pairs;
 * with it the lanes a run goes on and the table of machines, which creation and the launchers both read.  Private to the
 * library, like cpecan_ctx.h.
 */
#ifndef CPECAN_BATCH_H
#define CPECAN_BATCH_H

#include "cpecan_ctx.h"

#include "cpecan_asm.h"

#include <atomic>

struct SweepBuild; /* one compiled build of the throughput kernels (cpecan_sweep.h) */

/* one candidate pair on its way to the host: its coordinates.  With it goes the device's verdict (an int, see
 * cpecan_k_pack_pairs); the exponent (F + B) - totalProbability stays in HBM and is fetched for the few candidates the
 * host has to settle itself, and for callers that ask for it: 12 bytes per candidate cross PCIe instead of 20. */
struct PackedPair {
    int x, y;
};
#define CP_UNDECIDED_CAP 65536ull /* candidates per batch the host settles with its libm before it fetches exponents item by item */

struct cpecan_batch {
    cpecan_ctx *ctx = nullptr;
    std::shared_ptr<MemAccount> mem; /* the blocks of its DevBufs; part of its context's account (new_batch) */
    int64_t nItems = 0;
    int mode = 0, kernel = 0, flags = 0;
    DevParams P{};
    std::vector<DevItem> hItems;
    DevBuf<DevItem> items;
    DevBuf<int> bandL, bandR;
    DevBuf<long long> cellPrefix;
    DevBuf<char> chars, charsY; /* charsY: DNA batches (5-state machine) */
    Machine machine = STRAWMAN;
    bool wave5 = false; /* a DNA batch on the 5-state machine's wave kernels (choose_dispatch) */
    bool wave4 = false; /* a 4-state batch on that machine's wave kernels (CPECAN_FLAG_SM4_WAVE, choose_dispatch) */
    DevBuf<double> logNoise; /* vanilla and echelon batches: log(event noise), host libm */
    DevBuf<double> duration; /* echelon batches: per event the duration terms of 0..5 k-mers, host libm */
    DevBuf<long long> xEnd;  /* echelon batches: per item the X characters that belong to its sequence */
    DevBuf<int> kid;         /* HDP batches: k-mer id over the model's alphabet per X position */
    DevBuf<unsigned short> kidx;
    DevBuf<double> events;
    DevBuf<double> Fstore, Bstore, dbgB;
    DevBuf<double> Bring; /* systolic Baum-Welch: backward cells of one window per item */
    bool fused = false; /* (Dispatch::fused) strawMan E-step on the wave kernels (unless CPECAN_EXPECT_FUSED=0) or, with
                           CPECAN_FLAG_WORKGROUP_FUSED_ESTEP / CPECAN_FLAG_WIDE_BANDS_FUSED_ESTEP, on the workgroup kernels'
                           fused builds: expectations summed inside the sweep back, no B ring, no expectation kernel */
    DevBuf<long long> pairs;
    bool pairsLaidOut = true; /* false: lay_out_pairs was refused, `pairs` / `pairLogp` are not there */
    DevBuf<double> pairLogp;
    DevBuf<long long> nPairs, totXay, nTot, nCells;
    DevBuf<double> totVal;
    DevBuf<double> expect;
    DevBuf<double> expectSum; /* cpecan_hip_batch_sum_expectations: the models' blocks added up, made at its first call */
    DevBuf<int> workCounter;
    DevBuf<char> syStates, syScratch;
    DevBuf<int> bandTab; /* systolic kernels: (first, last) matrix column of every diagonal of every item */
    long long scratchBytes = 0;
    int nWindows = 0;
    DevBuf<double> track;
    DevBuf<long long> trackBase;
    long long ringDoubles = 0;
    int ringD = 0, maxLX = 0;
    int nWorkers = 0, maxWidth = 0;
    const SweepBuild *sy = nullptr; /* systolic path: the build of the kernels the batch runs on (Dispatch::build, choose_dispatch) */
    int device = 0;                    /* the context's device, kept for the destructor */
    int nModels = 0;
    int expectLen = CPECAN_EXPECTATION_LEN; /* doubles per model in `expect` */
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    /* systolic path: the batch runs as nGroups independent groups of alignments, each on a stream of
     * its own, so that the tail of one group's kernel overlaps the other groups' kernels (a launch
     * lasts as long as its slowest workgroup).  evStage: per group, one event after every kernel. */
    int nGroups = 1;
    /* (a wave batch of one group runs on lane sets instead: gStream empty, gStreamOwned false) */
    std::vector<hipStream_t> gStream, gStreamB; /* gStreamB: the wave kernels' backward sweeps (enqueue_sweeps, cpecan_run.hip) */
    bool postAside = false;            /* assembly sweeps: the totals and the decode of a window on the post lane, beside
                                          the next window's sweeps */
    std::vector<hipEvent_t> evPost;    /* ... done, per window */
    bool gStreamOwned = true;
    LaneSet *runLanes = nullptr; /* the lanes of its last run (a reference) */
    bool laneRun = false;        /* ... which went over their three streams: a follower is issued on them */
    long long modelEpoch = 0; /* the context's when the batch was created */
    int stateBytes = 0;
    std::vector<hipEvent_t> evStage, evJoin;
    hipEvent_t evFork = nullptr;
    std::vector<long long> hNPairs, hNTot, hNCells;
    /* aligned pairs as the callers get them: the device selects by the exponent with a margin, the host finishes
     * exp(), the threshold test and floor(p * 1e7) with the reference's libm (impl/pairwiseAligner.c:776-786) */
    std::vector<long long> hPairs; /* triples, packed per item at hPairBase */
    std::vector<double> hLogp;
    std::vector<long long> hPairBase;
    /* the way back to the host: the candidates of all items packed into one device buffer of 16-byte records and
     * copied in one piece into pinned memory */
    DevBuf<long long> packBase;
    DevBuf<PackedPair> packed;
    DevBuf<int> packedPost;
    DevBuf<long long> undecided;   /* cpecan_k_pack_pairs: [count | CP_UNDECIDED_CAP x (packed index, exponent bits)] */
    long long *hUndecided = nullptr; /* its pinned copy */
    PackedPair *hPacked = nullptr; /* hipHostMalloc */
    int *hPost = nullptr;          /* hipHostMalloc: the device's verdict per candidate (cpecan_k_pack_pairs) */
    size_t hPackedCap = 0;
    size_t hPackedBlock = 0, hPostBlock = 0, hUndecidedBlock = 0; /* the real sizes of those blocks (the allocator's cache) */
    int trackRow = CP_ROW; /* doubles per column of the track */
    bool countsValid = false, ran = false;
    bool packedInRun = false; /* the last run ended with cpecan_k_pack_base + cpecan_k_pack_pairs */
    bool compactPairs = false; /* every sequence of the batch is shorter than 65536 elements: a packed candidate crosses
                                  PCIe as (x | y << 16) and its verdict, 8 bytes instead of 12 */
    /* the hand-scheduled assembly sweeps (cpecan_asm.h): the host's plan of windows and band steps, the forward waves'
     * contexts */
    bool useAsm = false, asmBackward = false;
    int asmMaxWindows = 0;
    int asmCells = 0;          /* cells per lane of the assembly sweeps the batch runs (useAsm): 2 or 3 */
    std::string asmSetupError; /* why a batch planned for them does not run on them (a failed setup launch) */
    DevBuf<AsmPlanWin> planWin;
    DevBuf<AsmPlanCtl> planCtl;
    DevBuf<long long> planOff;
    DevBuf<char> asmCtx;
    DevBuf<unsigned> asmMasks;
};

/* (hidden like what cpecan_ctx.h declares; the struct above stands outside, as it did in cpecan_hip.hip: its implicit
 * destructor is among the library's weak exports, and the export list stays what it was) */
#pragma GCC visibility push(hidden)

/* The three streams a chain of batches runs on: forward (track, begin, the forward sweeps), back (the sweeps back) and
 * post (decode and re-sweep of a window, then the run's join, counts, packing and end event).  Every context has one;
 * a run behind a wave batch of one stream group (cpecan_hip_batch_run_after) is issued on the lanes that batch ran on,
 * so that a chain needs three hardware queues however many batches and contexts take part, and the order on each lane
 * orders the chain.  The forward lane is the context's first stream; back and post come with the context's first
 * wave batch of one group (the runtime deals its few hardware queues out in the order streams are made: a context
 * whose batches never use them -- the workgroup kernels of the E-step contexts -- leaves the queues to the others).
 * Held by reference: by its context, and by every batch whose last run went on it (until the batch runs again or is
 * destroyed). */
struct LaneSet {
    int device = 0;
    hipStream_t fwd = nullptr, back = nullptr, post = nullptr;
    std::mutex mu; /* held for the whole enqueue of one run: runs from two host threads do not interleave */
    std::atomic<int> refs{ 1 };
};

/* (cpecan_run.hip) */
hipError_t lanes_create(int device, LaneSet **out);
void lanes_release(LaneSet *L);
hipError_t lanes_sweeps(LaneSet *L); /* the back and post lanes, made when a batch that runs on them is created */

typedef const SweepBuild *const SweepFamily[4]; /* (a family's builds by rows, cpecan_hip.hip) */
/* One row of facts per machine (enum Machine, cpecan_ctx.h): what batch creation, the kernel choice and the launchers
 * know about a machine they read from its row.  Its models are the context's tables[machine]. */
enum XSource { X_KIDX, X_KID, X_CHARS }; /* what a kernel reads per X position: k-mer index, HDP k-mer id, nucleotide */
struct MachineRow {
    int states;        /* per cell */
    int expectLen;     /* doubles per model of the E-step's sums */
    int pairCapFactor; /* first guess of the pairs of an item, per element of lX + lY (ensure_counts re-runs a batch that
                          outgrows it).  16 for the HDP machine: it scores with linear densities (quirk Q6), its posteriors
                          are flat and far more cells pass the threshold (2887 pairs for a ~800-event read in the
                          reference's own test); and for echelon, which emits up to 15 pairs a cell */
    int xReach;        /* how far past lX a pair's x may lie (echelon: lX + 3), for compactPairs */
    const char *posteriorOnly; /* the refusal of an E-step (null: the machine has one) */
    const char *noDumps;       /* the refusal of CPECAN_FLAG_DEBUG_DUMP (null: it has cell dumps) */
    bool bandedEstep;          /* its E-step refuses CPECAN_FLAG_UNBANDED */
    /* the register-resident kernels: the machine's wave family and, where a batch may ask for it, its workgroup family
     * (null: none); per mode (CPECAN_MODE_POSTERIOR, CPECAN_MODE_EXPECTATIONS) the wide builds of the workgroup family
     * that serve it (null: none) and the flag they answer to: CPECAN_FLAG_WIDE_BANDS, CPECAN_FLAG_WIDE_BANDS_HDP,
     * CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP or CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP (0: none) */
    SweepFamily *wave, *workgroup;
    struct Wide {
        const SweepBuild *const *builds;
        int flag;
    } wide[2];
    bool ownChoice; /* its create call has no kernel argument: AUTO, or the general kernel with CPECAN_FLAG_GENERAL_KERNEL */
    /* the general kernel and what distinguishes its argument record */
    void (*general)(DevGeneralArgs, DevParams); /* (null: cpecan_k_generale, which takes a third record) */
    XSource x;
    bool yAux;       /* log(event noise) per event */
    int ldsMaxWidth; /* the widest band whose forward diagonals the general kernel keeps in LDS (0: it keeps none) */
};
extern const MachineRow MACHINES[N_MACHINES]; /* (cpecan_hip.hip, next to the tables of builds its rows point to) */

/* the end of a posterior run, queued on the stream it ends on before its end event: its candidates packed for the host
 * (cpecan_readback.hip) */
int pack_in_run(cpecan_batch *b, hipStream_t sEnd);
int lay_out_pairs(cpecan_batch *b); /* (cpecan_readback.hip; the run makes up for one that a memory limit refused) */
/* the batch's pinned blocks of the readback go back to the cache (cpecan_hip_batch_destroy) */
void release_readback(cpecan_batch *b);

#pragma GCC visibility pop

#endif
