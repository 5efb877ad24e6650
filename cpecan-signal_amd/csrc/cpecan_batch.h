/*
 * cpecan_batch.h -- the batch, as the two files that work on it see it: cpecan_hip.hip creates, runs and destroys it,
 * cpecan_readback.hip takes a finished run to the caller's counts and pairs.  Private to the library, like cpecan_ctx.h.
 */
#ifndef CPECAN_BATCH_H
#define CPECAN_BATCH_H

#include "cpecan_ctx.h"

#include "cpecan_asm.h"

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
    DevBuf<double> logNoise; /* vanilla and echelon batches: log(event noise), host libm */
    DevBuf<double> duration; /* echelon batches: per event the duration terms of 0..5 k-mers, host libm */
    DevBuf<long long> xEnd;  /* echelon batches: per item the X characters that belong to its sequence */
    DevBuf<int> kid;         /* HDP batches: k-mer id over the model's alphabet per X position */
    DevBuf<unsigned short> kidx;
    DevBuf<double> events;
    DevBuf<double> Fstore, Bstore, dbgB;
    DevBuf<double> Bring; /* systolic Baum-Welch: backward cells of one window per item */
    bool fused = false; /* strawMan E-step on the wave kernels (unless CPECAN_EXPECT_FUSED=0) or, with
                           CPECAN_FLAG_WORKGROUP_FUSED_ESTEP / CPECAN_FLAG_WIDE_BANDS_FUSED_ESTEP, on the workgroup kernels'
                           fused builds: expectations summed inside the sweep back, no B ring, no expectation kernel */
    DevBuf<long long> pairs;
    DevBuf<double> pairLogp;
    DevBuf<long long> nPairs, totXay, nTot, nCells;
    DevBuf<double> totVal;
    DevBuf<double> expect;
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
    const SweepBuild *sy = nullptr; /* systolic path: the build of the kernels the batch runs on (new_batch) */
    int device = 0;                    /* the context's device, kept for the destructor */
    int nModels = 0;
    int expectLen = CPECAN_EXPECTATION_LEN; /* doubles per model in `expect` */
    hipEvent_t ev0 = nullptr, ev1 = nullptr, ev2 = nullptr;
    /* systolic path: the batch runs as nGroups independent groups of alignments, each on a stream of
     * its own, so that the tail of one group's kernel overlaps the other groups' kernels (a launch
     * lasts as long as its slowest workgroup).  evStage: per group, one event after every kernel. */
    int nGroups = 1;
    /* (a wave batch of one group runs on lane sets instead: gStream empty, gStreamOwned false) */
    std::vector<hipStream_t> gStream, gStreamB; /* gStreamB: the wave kernels' backward sweeps (see batch_run) */
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

/* the end of a posterior run, queued on the stream it ends on before its end event: its candidates packed for the host
 * (cpecan_readback.hip) */
int pack_in_run(cpecan_batch *b, hipStream_t sEnd);
/* the batch's pinned blocks of the readback go back to the cache (cpecan_hip_batch_destroy) */
void release_readback(cpecan_batch *b);

#pragma GCC visibility pop

#endif
