/*
 * cpecan_sweep.h -- records shared by the throughput kernels (cpecan_kernel_wave.hip,
 * cpecan_kernel_systolic.hip: the sweeps, one build per object; cpecan_kernel_prep.hip: what a pass needs once) and the
 * C-ABI layer that sequences their launches.
 */
#ifndef CPECAN_SWEEP_H_
#define CPECAN_SWEEP_H_

#include "cpecan_device.h"

/* Per-alignment state handed between the forward-window and backward-window kernels. */
struct SyState {
    int d;            /* last forward diagonal completed */
    int tracedBackTo; /* as in getPosteriorProbsWithBanding (impl/pairwiseAligner.c:903) */
    int finished;     /* forward reached the last diagonal */
    int bandAi;       /* unused (kept for layout) */
    int winValid, winTop, winFrom, winTo, winAtEnd; /* traceback window for the backward kernel */
    int expectPending; /* Baum-Welch: the window's backward cells are in the B ring, not yet summed */
    long long nPairs, nTot, cells;
    long long clkShader, clkRef; /* shader-clock and 100 MHz reference ticks the alignment's forward sweeps took (the
                                    ratio is the clock the chip ran at under this load) */
};

/* The wave kernels' record: the forward kernel of launch w describes its window in win[w & 3] while the backward
 * kernel of launch w - 1 is working from the entry before and the post kernel of launch w - 2 may still be reading the
 * one before that (the assembly sweeps' schedule, cpecan_run.hip: they all run concurrently). */
struct WvWindow {
    int valid; /* 1: described by the forward kernel; 3: swept back, its totals and pairs are the post kernel's to do;
                  2: its candidates could not be trusted, the re-sweep kernel decodes it; 0: done */
    int top, from, to, atEnd;
    int nCand, nRefresh, pad; /* what the sweep back left in scratch for the post kernel */
    double est; /* estimate of the window's totalProbability: the forward cells of its top diagonal dotted with the
                   end vector the sweep back starts from (any fold order; it only steers the candidate test) */
};
struct WvState {
    int d;            /* last forward diagonal completed */
    int tracedBackTo; /* as in getPosteriorProbsWithBanding (impl/pairwiseAligner.c:903) */
    int finished;     /* forward reached the last diagonal */
    int expectPending; /* Baum-Welch: the window's backward cells are in the B ring, not yet summed */
    WvWindow win[4];
    long long nPairs, nTot, cells;
    long long clkShader, clkRef; /* shader-clock and 100 MHz reference ticks the alignment's forward sweeps took (the
                                    ratio is the clock the chip ran at under this load) */
};

/* per-window bookkeeping of one totalProbability refresh, kept in HBM scratch (private to the alignment) */
struct WinTotal {
    int t, xmin, xmax, nxmin, nxmax, second;
    double total;
};

/* What the stages of one pass over a batch read and write (host side only: the kernels keep their parameter lists, and
 * each launcher unpacks the record into one of them).  The C-ABI layer fills it once per run; the window index is a
 * launch argument of its own. */
struct SweepArgs {
    const DevItem *items;
    long long nItems;
    DevParams P;
    const int2 *bandTab;
    double *track; /* written by the track kernel, read by the sweeps */
    const long long *trackBase;
    int maxLX;
    const double *events;
    const unsigned short *kidx; /* per X position: k-mer index */
    const int *kid;             /* ... HDP batches: k-mer id over the model's alphabet (the HDP track kernel) */
    const double *models;       /* strawMan or vanilla tables, or the DevHdpModel records of an HDP batch */
    double *Fring;
    long long ringDoubles;
    int ringD;
    char *states;
    int stateBytes;
    long long *pairs;
    double *pairLogp;
    long long *totXay;
    double *totVal;
    char *scratch;
    long long scratchBytes;
    double *Bring; /* null unless the E-step keeps its backward cells */
    int bringRow;  /* doubles per diagonal of it */
    double *expect;
    long long *nPairs, *nTot, *nCells; /* the counts kernel's */
    int withSwitch; /* some model lets gap Y switch to gap X: the builds with that term */

    /* the record of the stream group of n alignments from i0 on: the kernels index what is kept per alignment by
     * blockIdx, so those bases shift; everything else is addressed through the item */
    SweepArgs slice(long long i0, long long n) const {
        SweepArgs a = *this;
        a.items += i0;
        a.nItems = n;
        a.trackBase += i0;
        a.Fring += i0 * ringDoubles;
        a.states += i0 * stateBytes;
        a.scratch += i0 * scratchBytes;
        if (a.Bring) a.Bring += i0 * (long long) ringD * bringRow;
        return a;
    }
};

typedef int (*SweepLaunch)(hipStream_t stream, const SweepArgs &a, int window);

/* the once-per-pass pieces of a machine on a kernel family (cpecan_kernel_prep.hip): the track before the sweeps, the
 * counts after them */
struct SweepMachine {
    int stateBytes;      /* per alignment: SyState or WvState */
    int trackRowDoubles; /* per matrix column of the track */
    int (*launch_track)(hipStream_t stream, const SweepArgs &a); /* (and the states cleared) */
    int (*launch_counts)(hipStream_t stream, const SweepArgs &a);
};
extern "C" const SweepMachine cpecan_systolic_machine, cpecan_systolic_machine_vanilla, cpecan_systolic_machine_hdp, cpecan_wave_machine,
    cpecan_wave_machine_hdp, cpecan_wave_machine_vanilla;

/* ... and what the same file has for batch creation and the self-tests: per X position the k-mer index, or the k-mer id
 * over an HDP's alphabet (up to 16 characters, eight to a word); the division self-test; the shader clock the forward
 * sweeps of the last run saw */
extern "C" __global__ void cpecan_k_kmer_index(const char *chars, long long n, unsigned short *kidx);
extern "C" __global__ void cpecan_k_hdp_kmer_id(const char *chars, long long n, unsigned long long alphabet,
                                                unsigned long long alphabetHi, int alphabetSize, int *kid);
extern "C" int cpecan_systolic_divtest(hipStream_t stream, long long n, unsigned long long seed, unsigned long long *bad);
extern "C" int cpecan_wave_shader_clock_mhz(hipStream_t stream, const void *states, long long nItems, double *mhz);

enum { SWEEP_STRAWMAN, SWEEP_HDP, SWEEP_VANILLA };

/* the symbols of a build carry its machine's tag and its number: SWEEP_SYM(cpecan_k_sy_forward, he, 6) is
 * cpecan_k_sy_forward_he6 (two levels, so that a number given with -D is expanded before it is pasted) */
#define SWEEP_SYM_(n, tag, k) n##_##tag##k
#define SWEEP_SYM(n, tag, k) SWEEP_SYM_(n, tag, k)

/* One compiled build of the throughput kernels, defined next to them: cpecan_systolic_build<suffix> in
 * cpecan_kernel_systolic.hip, cpecan_wave_build<suffix> in cpecan_kernel_wave.hip, one per build of the Makefile's list
 * (SY_BUILDS, WV_BUILDS, and the unsuffixed four-wave build) */
struct SweepBuild {
    int rows;    /* waves per workgroup (workgroup family) or cells per lane (wave family) */
    bool wave;   /* one wave per alignment */
    int machine; /* SWEEP_STRAWMAN, SWEEP_HDP, SWEEP_VANILLA */
    const SweepMachine *once; /* ... and its once-per-pass pieces on this family */
    int maxWidth;        /* widest band, in k-mers */
    int ringRowDoubles;  /* per diagonal of the forward ring */
    int bringRowDoubles; /* ... of the ring of backward cells */
    long long (*scratch_bytes)(int ringD);    /* HBM scratch per alignment */
    long long (*fx_scratch_bytes)(int ringD); /* ... and what fused expectations add behind it (null: none) */
    SweepLaunch forward;
    SweepLaunch backward;    /* the sweep back of a window and what follows it (totals, decode, re-sweep) */
    SweepLaunch backward_fx; /* the E-step with the expectations summed inside the sweep back (null: none; the wave
                                builds of the strawMan machine, and the workgroup family's _f and the vanilla machine's
                                _vf builds and the HDP machine's _hf builds, which have no other: their expect is null,
                                and the _vf and _hf builds, which only a batch of expectations reaches, have no backward
                                either) */
    SweepLaunch expect;      /* the E-step from the ring of backward cells */
    SweepLaunch post_asm;    /* what follows the assembly sweep back of a window (null: no assembly sweeps) */
};

#endif
