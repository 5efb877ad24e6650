/*
 * cpecan_kernel_systolic.hip -- the throughput kernels: banded forward / backward / posterior DP
 * with the anti-diagonal wavefront of the recurrence held in registers.
 *
 * Mapping (designed for CDNA4's 64-lane waves, not translated from anything):
 *   - one workgroup of SY_R waves per alignment (256 threads in the four-wave build); lanes own reference k-mers,
 *     not DP cells: slot s = x mod 64*SY_R is lane s % 64 of wave s / 64 (bands up to 64*SY_R - 8 k-mers wide).  A k-mer's 17
 *     emission constants stay in its lane's VGPRs while x is inside the band.
 *   - one loop iteration = one anti-diagonal.  Forward: a cell needs (x-1,y) and (x-1,y-1) from the
 *     lane below (one DPP wave-shift per value) and (x,y-1) from itself; only lane 0 of a wave
 *     takes its neighbour from the wave below through 40 bytes of LDS (one LDS-only barrier per
 *     diagonal).  The event a lane scores also moves up one lane per diagonal.
 *   - backward is the mirror image (messages travel down one lane); it is a gather, with the
 *     reference's scatter order of accumulation kept per state (see cpecan_kernel_general.hip).
 *   - forward cells go to HBM once into a per-alignment ring holding one traceback window
 *     ([diagonal][wave][Fm,Fx,Fy,pm,py][lane]) and are read once by the sweep back.
 *   - neither sweep waits for a global load inside its loop: the forward sweep stages its inputs
 *     (events, k-mer rows, band) in LDS every 32 diagonals, the backward sweep fetches ring rows
 *     four diagonals ahead with the loop unrolled by four (see Feed, BandFeed, backward_window).
 *   - the posterior decode works from candidate lists the sweep back collects (backward_window).
 *   - two kernels per traceback window, launched by the C-ABI layer (cpecan_hip.hip): forward to
 *     the next traceback point, then backward + decode of that window; per-alignment state
 *     (SyState) and the ring carry over.
 * MFMA is not used: the recurrence is a scan with an approximate log-add, not a contraction.
 *
 * Numerics: identical to the general kernel and the CPU oracle, bit for bit.  The only algebraic
 * change is the division (x - mu) / sigma, done as a Markstein-corrected multiply by the
 * host-rounded reciprocal (two fused multiply-adds), which returns the correctly rounded quotient
 * (tests/test_systolic_gpu.py checks it against IEEE division on 10^8 operands).
 *
 * -DSY_ABLATE_* and -DSY_PROFILE are timing-study switches (tools/ablate.sh, tools/prof.sh); the
 * ablations compute wrong results by construction and are never built into the product.
 */
#include "cpecan_device.h"
#include "cpecan_lanes.h"
#include "cpecan_sweep.h"

#ifndef SY_R
#define SY_R 4 /* waves per workgroup: 4 (bands up to 248 k-mers) or 3 (up to 184; five workgroups fit a CU) */
#endif
#define SY_P (64 * SY_R)
/* this file is compiled once per build of the Makefile's list (SY_BUILDS, and once with neither -DSY_R nor a suffix:
 * the four-wave strawMan build): with 1..4 waves per workgroup for bands up to 56, 120, 184, 248 k-mers, with 6 and 8
 * for the wide bands (376 and 504), and with the switches described below.  Every build holds the sweeps -- a forward, a
 * backward and, where the machine has its E-step here, an expectation kernel -- their launchers and one SweepBuild
 * record; what does not depend on the build (track, counts, the machines' records) is cpecan_kernel_prep.hip's */
/* -DSY_VANILLA: the same two sweeps for the 3-state vanilla signal machine (stateMachine3Vanilla_cellCalculate,
 * impl/stateMachine.c:1368-1409), posterior decode only, with four, six and eight waves per workgroup (bands of up to
 * 248, 376 and 504 k-mers; symbols suffixed _v4, _v6, _v8).  A lane holds the 21 doubles of its k-mer's row of the
 * vanilla track (cpecan_k_wv_track_vanilla): two tables of Gaussian level and inverse-Gaussian noise
 * constants and the five log transition probabilities of the column's skip bin, so transitions are per lane, not
 * per wave; a_ym, a_yy and the end vector come from the model header.  These builds have no ring of backward cells and
 * no expectation kernel: the E-step of this machine at these widths is the _ve builds' (below). */
/* -DSY_HDP: the forward sweep of the 3-state HDP signal machine (stateMachine3HDP_cellCalculate, impl/stateMachine.c:
 * 1338-1370) with six and eight waves per workgroup (bands of 249..376 and 377..504 k-mers; symbols suffixed _h6, _h8;
 * the HDP wave builds reach 248, so there is no four-wave build), posterior decode only.  One spline density of the
 * NanoporeHDP is the match and the gap-Y emission, the gap-X emission is a flat log(0.1): a slot keeps one value, the
 * offset of its k-mer's table row, and the gap-X sums are the same for every k-mer, so they are wave-uniform.  The
 * sweep back, the totals and the decode are the strawMan's source unchanged: they read the nine transitions from the
 * head of the model record (DevHdpModel starts with them; only the stride between models differs, which is why these
 * builds compile the sweep back themselves) and the gap-X emission from entry CP_GAPX of the track row
 * (cpecan_k_sy_track_hdp writes log(0.1) there). */
/* -DSY_HDP -DSY_ESTEP: the HDP machine's E-step at the same two widths, in objects of their own (symbols suffixed _he6,
 * _he8; the _h6 / _h8 objects keep their device code).  E-step only: SY_MODE(P) is the constant 1, so the forward sweep
 * keeps every state of every diagonal, the sweep back parks its cells in the B ring, and the candidate lists and both
 * decodes fold away; cpecan_k_sy_expect is compiled in its HDP form (nine transitions and the likelihood, no k-mer bins,
 * event-to-k-mer assignments). */
/* -DSY_VANILLA -DSY_ESTEP: the vanilla machine's E-step with four, six and eight waves per workgroup (bands of 185..248,
 * 249..376 and 377..504 k-mers), in objects of their own (symbols suffixed _ve4, _ve6, _ve8; the _v4 / _v6 / _v8 objects
 * keep their device code).  E-step only, as the _he builds: SY_MODE(P) is the constant 1.  This machine's E-step reads
 * one backward value per cell, B.gapX, so the sweep back parks that one alone: a B ring of [diagonal][wave][lane], a
 * third of the strawMan builds'.  cpecan_k_sy_expect is compiled in its vanilla form (30 + 30 skip bins and the
 * likelihood: match -> gap X and gap X -> gap X, from the cell's lower neighbour). */
/* -DSY_FUSED: the strawMan machine's E-step with its expectations summed inside the sweep back, with one to four, six
 * and eight waves per workgroup, in objects of their own (symbols suffixed _f1.._f4, _f6, _f8; the _r1.._r8 and the
 * unsuffixed objects keep their device code).  _f6 and _f8 serve the bands of _r6 and _r8 (249..376 and 377..504
 * k-mers); nothing of the fused pass depends on the number of waves beyond SY_R and SY_P: the segment records are
 * [segment][wave][8] and [segment][A | B][slot] (sy_fx_bytes), the hit masks (SY_MSK) belong to the decode, which these
 * builds do not have, and the band ring is staged again for a second sweep by the whole workgroup.  _f6 alone keeps a
 * lane's eight sums in LDS (SY_FX_LDS).  E-step only: SY_MODE(P) is the constant 1, so the forward sweep keeps every
 * state of every diagonal.
 * The sweep back fetches F.gapX and F.gapY of a row with its F.match and forms, per cell, the terms of
 * diagonalCalculation_Expectations (see fx_terms in backward_window): no ring of backward cells, no expectation kernel.
 * The terms are taken against the window's estimated total and kept per refresh segment (FxRecords); after phase T they
 * are scaled to the exact totals and added to the model's sums (fx_finish), and a window whose estimate cannot be
 * trusted is swept back once more, in the same launch, against the exact totals. */
/* -DSY_VANILLA -DSY_FUSED: the vanilla machine's E-step with its expectations summed inside the sweep back, with four,
 * six and eight waves per workgroup (the bands of _ve4 / _ve6 / _ve8), in objects of their own (symbols suffixed
 * _vf4, _vf6, _vf8; the _ve objects keep their device code).  The forward sweep is the _ve builds'.  This machine collects two terms per
 * cell and no transition, both from the cell's lower neighbour (cpecan_k_sy_expect, vanilla form), so the sweep back
 * fetches F.gapX beside F.match, takes B.gapX and the column's a_mx / a_xx apart down the lanes (the recurrence's sums
 * are formed by the receiver: the same doubles) and keeps (column, beta, alpha) per slot and refresh segment, in
 * registers: no ring of backward cells, no expectation kernel.  The estimate, the segments' scaling, the second sweep
 * and DevParams::expectResweep are the strawMan fused builds' (above); fx_finish adds through 60 bins in LDS. */
/* -DSY_HDP -DSY_FUSED: the HDP machine's E-step with its expectations summed inside the sweep back, with six and eight
 * waves per workgroup (the bands of _he6 / _he8), in objects of their own (symbols suffixed _hf6, _hf8; the
 * _he objects keep their device code).  The forward sweep is the _he builds'.  The sums are the strawMan fused builds' without the k-mer bins
 * (no g, no c records: SY_FX_G 0), into the model's nine transitions and its likelihood.  The machine's event-to-k-mer
 * assignments (cpecan_k_sy_expect, HDP form) come from the same sweep: in the middle block it parks the target cell, the
 * from-state and the exponent s before the total is subtracted, wherever s lies within SY_CAND_SLACK of the threshold
 * against the estimate, in the candidate lists the posterior builds keep in the window scratch; after phase T a
 * selection phase takes e = s - total of the target diagonal's segment and appends where exp(e) reaches the threshold --
 * the subtraction is the last operation of the ring path's expression, so triples and exponents are its bit for bit.
 * One redo rule for sums and assignments: a window with a total that is not finite or more than SY_CAND_SLACK from the
 * estimate, with a list that overflowed, of a batch whose threshold has no logarithm, or that DevParams::expectResweep
 * names is swept once more against the exact totals, and that sweep emits the assignments in its loop. */
#if defined(SY_FUSED) && defined(SY_HDP) && !defined(SY_ESTEP) && !defined(SY_VANILLA)
#define SY_HDP_FUSED
#endif
#if defined(SY_FUSED) && defined(SY_ESTEP)
#error "SY_FUSED: a build of the strawMan machine or, with SY_VANILLA or SY_HDP alone, of that machine"
#elif defined(SY_HDP) && defined(SY_VANILLA)
#error "SY_HDP and SY_VANILLA are builds of their own"
#elif defined(SY_ESTEP) && !defined(SY_HDP) && !defined(SY_VANILLA)
#error "SY_ESTEP: the E-step builds of the HDP machine (-DSY_HDP) and of the vanilla machine (-DSY_VANILLA)"
#elif defined(SY_ESTEP) && defined(SY_HDP) && SY_R != 6 && SY_R != 8
#error "SY_HDP SY_ESTEP: 6 or 8 waves per workgroup"
#elif defined(SY_HDP) && SY_R != 6 && SY_R != 8
#error "SY_HDP: 6 or 8 waves per workgroup"
#elif defined(SY_VANILLA) && SY_R != 4 && SY_R != 6 && SY_R != 8
#error "SY_VANILLA: 4, 6 or 8 waves per workgroup"
#elif SY_R != 1 && SY_R != 2 && SY_R != 3 && SY_R != 4 && SY_R != 6 && SY_R != 8
#error "SY_R: 1, 2, 3, 4, 6 or 8 waves per workgroup"
#endif
/* a symbol's suffix: the machine's tag and the number of waves; the strawMan's four-wave build alone has none */
#if defined(SY_FUSED) && defined(SY_VANILLA)
#define SY_SYM(n) SWEEP_SYM(n, vf, SY_R)
#elif defined(SY_HDP_FUSED)
#define SY_SYM(n) SWEEP_SYM(n, hf, SY_R)
#elif defined(SY_FUSED)
#define SY_SYM(n) SWEEP_SYM(n, f, SY_R)
#elif defined(SY_ESTEP) && defined(SY_VANILLA)
#define SY_SYM(n) SWEEP_SYM(n, ve, SY_R)
#elif defined(SY_ESTEP)
#define SY_SYM(n) SWEEP_SYM(n, he, SY_R)
#elif defined(SY_HDP)
#define SY_SYM(n) SWEEP_SYM(n, h, SY_R)
#elif defined(SY_VANILLA)
#define SY_SYM(n) SWEEP_SYM(n, v, SY_R)
#elif SY_R != 4
#define SY_SYM(n) SWEEP_SYM(n, r, SY_R)
#else
#define SY_SYM(n) n
#endif
#if defined(SY_VANILLA) /* the vanilla row does not fit 128 VGPRs: whatever occupancy the allocation lands on */
/* (the _ve sweep back lands on 124..128; the fused one, _vf, on 141..145: the four F.gapX in flight, the two sums, their
 * column and the record addresses are seventeen registers the 128 do not have -- held to four waves per SIMD it spills
 * twelve to fourteen, eight with the sums in LDS, six to twelve with three of the row's transitions there too -- so it
 * runs three waves per SIMD) */
#define SY_BACKWARD_ATTR
#elif defined(SY_FUSED) && SY_R == 6 && !defined(SY_FX_REG_SUMS)
/* the six-wave fused sweep back with its eight sums in LDS (SY_FX_LDS below) fits three waves per SIMD without a spill (165
 * VGPRs): two six-wave workgroups share a CU, as on _r6.  Left alone it takes 173, and 179 with the sums in registers.
 * The HDP machine's _hf6 keeps both, the sums in LDS and the three waves: 164 VGPRs, no spill, 33136 bytes of static LDS
 * (two workgroups: 66 KB of the CU's 160), against 178 with the sums in registers and no occupancy forced -- one
 * workgroup to a CU where _he6 (119) has two.  _hf8 lands on 178 by itself (below), as _f8 on 179: two waves per SIMD,
 * one eight-wave workgroup to a CU; its static LDS is _he8's, 10896 bytes. */
#define SY_BACKWARD_ATTR __attribute__((amdgpu_waves_per_eu(3, 3)))
#elif defined(SY_FUSED) /* nor do the fused sweep's accumulators and wider fetch buffers: no occupancy is forced */
#define SY_BACKWARD_ATTR
#elif SY_R == 1 || SY_R == 8 /* the one-wave and the eight-wave backward kernel land on 129 VGPRs by themselves: hold
                            * them to four waves per SIMD (128; two eight-wave workgroups then share a CU) */
#define SY_BACKWARD_ATTR __attribute__((amdgpu_waves_per_eu(4, 4)))
#else
#ifdef SY_FORCE_WAVES
#define SY_BACKWARD_ATTR __attribute__((amdgpu_waves_per_eu(SY_FORCE_WAVES, SY_FORCE_WAVES)))
#else
#define SY_BACKWARD_ATTR
#endif
#endif
#if SY_R == 4 || SY_R == 8 /* a power of two: masks */
#define SY_WAVE_OF(x) (((x) >> 6) & (SY_R - 1)) /* the wave that owns k-mer x (x >= 0) */
#define SY_WMOD(v) ((v) & (SY_R - 1))           /* a difference of wave indices, any sign, into 0..SY_R-1 */
#define SY_SLOT(x) ((x) & (SY_P - 1))
#else
#define SY_WAVE_OF(x) (((x) >> 6) % SY_R)
#define SY_WMOD(v) ((((v) % SY_R) + SY_R) % SY_R)
#define SY_SLOT(x) ((x) % SY_P)
#endif
#ifdef SY_VANILLA
#define SY_ROW CP_WV_ROW_VANILLA /* doubles per column of the vanilla track */
#define SY_NPRM 21   /* ... of which a slot keeps all but the last (the bin itself, E-step only) */
#define SY_TR 16     /* first of the row's five log transition probabilities: a_mx, a_xx, a_mm, a_xm, a_my */
#define SY_EVW 4     /* doubles per staged event: mean, noise, 1 / noise, log(noise) */
#define SY_MODEL_DOUBLES ((long long) CP_VMODEL_STRIDE)
#define SY_MACHINE_ID SWEEP_VANILLA /* (the build's record, at the end of the file) */
#define SY_MACHINE cpecan_systolic_machine_vanilla
#if defined(SY_ESTEP) || defined(SY_FUSED)
#define SY_MODE(P) 1 /* E-step only */
#else
#define SY_MODE(P) 0 /* posterior decode only */
#endif
#elif defined(SY_HDP)
#define SY_ROW CP_ROW /* the strawMan track's row: entry 0 the k-mer's table row offset, entry CP_GAPX log(0.1) */
#define SY_NPRM 1    /* a slot keeps the table row offset */
#define SY_EVW 2     /* doubles per staged event: grid cell of its mean, offset in the cell */
#define SY_MODEL_DOUBLES ((long long) (sizeof(DevHdpModel) / sizeof(double)))
#define SY_MACHINE_ID SWEEP_HDP
#define SY_MACHINE cpecan_systolic_machine_hdp
#if defined(SY_ESTEP) || defined(SY_FUSED)
#define SY_MODE(P) 1 /* E-step only */
#else
#define SY_MODE(P) 0 /* posterior decode only */
#endif
#define SY_HDP_GAPX CP_HDP_GAPX
#else
#define SY_ROW CP_ROW
#define SY_NPRM 17
#define SY_EVW 2     /* doubles per staged event: mean, noise */
#define SY_MODEL_DOUBLES ((long long) CP_MODEL_STRIDE)
#define SY_MACHINE_ID SWEEP_STRAWMAN
#define SY_MACHINE cpecan_systolic_machine
#ifdef SY_FUSED
#define SY_MODE(P) 1 /* E-step only */
#else
#define SY_MODE(P) (P).mode
#endif
#endif
#if ((defined(SY_VANILLA) || defined(SY_HDP)) && !defined(SY_ESTEP)) || defined(SY_FUSED)
#define SY_NO_ESTEP /* these builds have no expectation kernel and no ring of backward cells */
#endif
/* SY_ESTEP_BY(fused, ring): a field of the build's record that depends on its E-step -- summed inside the sweep back,
 * taken from the ring of backward cells, or none (null) */
#if defined(SY_FUSED)
#define SY_ESTEP_BY(fused, ring) fused
#elif defined(SY_NO_ESTEP)
#define SY_ESTEP_BY(fused, ring) nullptr
#else
#define SY_ESTEP_BY(fused, ring) ring
#endif
#ifdef SY_FUSED
#define SY_FX true
#else
#define SY_FX false
#endif
/* SY_FXQ(x, y): arguments only the fused builds' fetch and step take (a row's F.gapX and F.gapY; the vanilla machine's
 * terms start at no gap-Y cell: F.gapX alone) */
#if defined(SY_FUSED) && defined(SY_VANILLA)
#define SY_FXQ(x, y) , x
#elif defined(SY_FUSED)
#define SY_FXQ(x, y) , x, y
#else
#define SY_FXQ(x, y)
#endif
/* SY_FX_LDS: the fused sweep back keeps a lane's eight transition sums in LDS, [sum][thread], instead of sixteen VGPRs --
 * the six-wave build only: up to four waves no occupancy is in reach of sixteen registers, at eight only 128 registers
 * would bring a second workgroup to the CU.  -DSY_FX_REG_SUMS (a timing-study switch, like SY_ABLATE_*, with the same
 * results) keeps them in registers there too */
#if defined(SY_FUSED) && !defined(SY_VANILLA) && SY_R == 6 && !defined(SY_FX_REG_SUMS)
#define SY_FX_LDS
#endif
#define SY_FX_EST_BOUND 30.0 /* nats an exact total may lie from the estimate the fused sums were taken against */
#define SY_FX_ZERO (-746.0)  /* exp() below this is +0 in double precision (the least denormal is exp(-744.44)) */
/* per cell in the ring of backward cells: the three states, or the one the vanilla E-step reads (gap X) */
#if defined(SY_VANILLA)
#define SY_BRING_VALUES 1
#else
#define SY_BRING_VALUES 3
#endif
#ifdef SY_NO_ESTEP
#define SY_BRING_ROW_DOUBLES 0
#else
#define SY_BRING_ROW_DOUBLES (SY_R * SY_BRING_VALUES * 64) /* per diagonal */
#endif
#define SY_PREFETCH 4     /* diagonals the backward sweep fetches ahead (== its unroll factor) */
#define SY_CAND_SLACK 0.25 /* candidates: cells within this (log units) below the posterior threshold */
#define SY_CAND_PER_DIAG 4 /* candidate capacity per wave, in records per ring diagonal */
#define SY_DECODE_U 2     /* diagonals per batch of the posterior decode */
#define SY_EXPECT_CHUNKS 8 /* workgroups that share one window's diagonals in the expectation pass */
#define SY_RING_VALUES 5 /* per cell in the forward ring: Fm, Fx, Fy, match emission, gap-Y emission */
/* hit masks (one per wave) the decode keeps per diagonal in scratch: a power of two, so that a lane finds its
 * (diagonal, wave) by shift and mask -- four whatever SY_R is up to four waves, eight for the wide builds */
#if SY_R <= 4
#define SY_MSK_SHIFT 2
#else
#define SY_MSK_SHIFT 3
#endif
#define SY_MSK (1 << SY_MSK_SHIFT)

#ifdef SY_PROFILE
/* timing build only: cycles per section of the forward step, summed over all waves (16 counters per wave), then the
 * 16 counters of the sweep back: 80 in all up to four waves, 16 * SY_R + 16 in the wide builds */
#define SY_PROF_B (16 * (SY_R > 4 ? SY_R : 4))
#define SY_PROF_N (SY_PROF_B + 16)
__device__ unsigned long long SY_SYM(sy_prof)[SY_PROF_N];
#define sy_prof SY_SYM(sy_prof)
#define PROF_DECL unsigned long long prof_[12] = {0,0,0,0,0,0,0,0,0,0,0,0}, tprev_ = __builtin_readcyclecounter(); bool pact_ = false;
#define PROF(k) { const unsigned long long now_ = __builtin_readcyclecounter(); if (pact_) prof_[k] += now_ - tprev_; else prof_[9] += now_ - tprev_; tprev_ = now_; }
#define PROF_ACTIVE(a) { pact_ = (a); if (pact_) prof_[10]++; else prof_[11]++; }
#define PROF_FENCE(x) asm volatile("" : "+v"(x));
#define BPROF_DECL unsigned long long bt_[9]; for (int k_ = 0; k_ < 9; k_++) bt_[k_] = 0; bt_[0] = __builtin_readcyclecounter(); const unsigned long long rt0_ = __builtin_amdgcn_s_memrealtime();
#define BPROF(k) bt_[k] = __builtin_readcyclecounter();
#define BPROF_FLUSH if (threadIdx.x == 0) { for (int k_ = 0; k_ < 8; k_++) atomicAdd(&sy_prof[SY_PROF_B + k_], bt_[k_ + 1] - bt_[k_]); atomicMax(&sy_prof[SY_PROF_B + 11], bt_[8] - bt_[0]); { const unsigned long long rd_ = __builtin_amdgcn_s_memrealtime() - rt0_; atomicAdd(&sy_prof[SY_PROF_B + 12], rd_); atomicMax(&sy_prof[SY_PROF_B + 13], rd_); } atomicAdd(&sy_prof[SY_PROF_B + 8], 1ull); atomicAdd(&sy_prof[SY_PROF_B + 9], (unsigned long long) (sh.scan != 0)); { int nc_ = 0; for (int w_ = 0; w_ < SY_R; w_++) nc_ += sh.cnt[1][w_][0]; atomicAdd(&sy_prof[SY_PROF_B + 10], (unsigned long long) nc_); } }
#define PROF_FLUSH(wave) if ((threadIdx.x & 63) == 0) { for (int k_ = 0; k_ < 12; k_++) atomicAdd(&sy_prof[(wave) * 16 + k_], prof_[k_]); }
#else
#define PROF_DECL
#define PROF(k)
#define PROF_ACTIVE(a)
#define PROF_FENCE(x)
#define PROF_FLUSH(wave)
#define BPROF_DECL
#define BPROF(k)
#define BPROF_FLUSH
#endif

namespace {

struct Shared {
    double coef[64];         /* lookup() cubics [c3,c2,c1,c0] by n = ceil(2d), 0..15: one ds_read_b128 pair per logAdd */
    double xch[2][SY_R][8];  /* boundary-lane values, double-buffered by diagonal parity */
    double vbuf[SY_P];       /* phase T: per-thread fold results; the sweep's estimate of the total */
    double wbuf[SY_P];       /* decode: partial hit counts */
    double total;
    int cnt[2][SY_R][2];     /* aligned-pair counts per wave, double-buffered */
    int item;
    int scan;                /* this window's posteriors must be decoded by the full scan */
#if defined(SY_FUSED) && !defined(SY_VANILLA) && !defined(SY_HDP)
    int fxRedo;              /* this window's sums must be taken again, against the exact totals */
#define SY_FX_REDO(sh) (sh).fxRedo
#elif defined(SY_FUSED)
/* (the vanilla and the HDP fused builds keep the forward sweep's LDS that of the _ve / _he builds: the flag lives in the
 * decode's first pair count, which no E-step build reads or writes) */
#define SY_FX_REDO(sh) (sh).cnt[0][0][0]
#endif
};

/*
 * Inputs of the forward sweep, staged in LDS.  Inside the sweep a wave must never wait on a
 * global load: vmcnt counts loads and stores in one in-order queue, so waiting for any load also
 * waits for the acknowledgement of every ring store issued before it -- a full HBM round trip per
 * anti-diagonal.  Events and k-mer constants are therefore fetched in bulk once every SY_FEED
 * diagonals, for the next two such blocks (both move by at most one index per diagonal), and the
 * sweep itself only reads LDS.
 */
#define SY_FEED 32
#define SY_FEED_EV 128  /* ring of events, by event index            */
#define SY_FEED_ROW 64  /* ring of k-mer constant rows, by k-mer index */
#ifdef SY_HDP
#define SY_FEEDW 1 /* doubles of a track row the ring keeps: the table row offset */
#else
#define SY_FEEDW SY_ROW
#endif
struct Feed {
    double ev[SY_FEED_EV * SY_EVW];
    double row[SY_FEED_ROW * SY_FEEDW];
};

/* the work item as wave-uniform (scalar) values: everything derived from it -- band geometry, loop
 * bounds, base addresses -- then stays on the scalar unit instead of occupying vector lanes */
__device__ __forceinline__ DevItem uniform_item(const DevItem &s) {
    DevItem d;
    d.lX = uni64(s.lX); d.lY = uni64(s.lY); d.xOff = uni64(s.xOff); d.yOff = uni64(s.yOff);
    d.anchorOff = uni64(s.anchorOff); d.nAnchors = uni64(s.nAnchors); d.diagBase = uni64(s.diagBase); d.cellBase = 0;
    d.nCells = 0; d.pairBase = uni64(s.pairBase); d.pairCap = uni64(s.pairCap);
    d.totBase = uni64(s.totBase); d.totCap = uni64(s.totCap); d.bwsBase = 0;
    d.model = uni(s.model); d.raggedL = uni(s.raggedL); d.raggedR = uni(s.raggedR); d.maxWidth = 0;
    return d;
}

/* Workgroup barrier that orders LDS traffic only.  __syncthreads() would also drain every global
 * store of the forward ring (s_waitcnt vmcnt(0)) on each anti-diagonal; nothing the waves exchange
 * inside an alignment goes through global memory, so only lgkmcnt has to reach zero. */
__device__ __forceinline__ void lds_barrier() {
#ifdef SY_ABLATE_BARRIER
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#else
    asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
#endif
}

/* logAdd (impl/pairwiseAligner.c:238-255), branch-free and bit-identical: hi/lo are the operands
 * as the reference's two branches order them; its "smaller operand is -inf" and ">= 7.5" exits both
 * yield hi, and (-inf) - (-inf) = NaN fails d < 7.5 exactly like those exits.  The cubic's four
 * float-literal coefficients come from a 128-byte LDS table indexed by the piece (<=1, <=2.5,
 * <=4.5, else): two ds_read_b128 instead of a 24-select chain. */
__device__ __forceinline__ double ladd(double x, double y, const double *coef) {
#ifdef SY_ABLATE_LADD
    return x > y ? x : y;
#endif
    double hi, lo;
    /* plain v_max/v_min: operands are never NaN, so the canonicalising pre-ops fmax()/fmin() emit
     * are dead weight in a loop that is bound by instruction issue */
    asm("v_max_f64 %0, %1, %2" : "=v"(hi) : "v"(x), "v"(y));
    asm("v_min_f64 %0, %1, %2" : "=v"(lo) : "v"(x), "v"(y));
    const double d = hi - lo;
    /* the piece of lookup() (d <= 1, <= 2.5, <= 4.5, else) from n = ceil(2d): the thresholds are
     * multiples of 1/2 and 2d is exact, so d > 1 <=> n >= 3, d > 2.5 <=> n >= 6, d > 4.5 <=> n >= 10;
     * the LDS table holds the cubic of n's piece at entry n (0..15), so no comparison is needed.
     * NaN (both operands -inf) converts to 0, d >= 7.5 is clamped: either way the cubic is discarded. */
    int n;
#ifdef SY_ABLATE_COEF
    n = 0;
#else
    asm("v_cvt_i32_f64 %0, %1" : "=v"(n) : "v"(__builtin_ceil(d + d)));
    n = n < 15 ? n : 15;
#endif
    /* one LDS address, two 16-byte reads (the compiler would form two addresses) */
    const unsigned a = (unsigned) (size_t) (const __attribute__((address_space(3))) double *) coef + n * 32u;
    double2 c32, c10;
    asm volatile("ds_read_b128 %0, %2\n\tds_read_b128 %1, %2 offset:16\n\ts_waitcnt lgkmcnt(0)"
                 : "=&v"(c32), "=&v"(c10) : "v"(a));
    const double r = ((c32.x * d + c32.y) * d + c10.x) * d + c10.y + lo;
    return d < 7.5 ? r : hi;
}
__device__ __forceinline__ void init_coef(double *coef) {
    const float t[16] = CP_LOOKUP_CUBICS;
    /* entry n = ceil(2d) carries the cubic [c3,c2,c1,c0] of the piece d falls in */
    if (threadIdx.x < 64) {
        const int n = threadIdx.x >> 2, piece = n <= 2 ? 0 : n <= 5 ? 1 : n <= 9 ? 2 : 3;
        coef[threadIdx.x] = (double) t[piece * 4 + (threadIdx.x & 3)];
    }
}

#ifdef SY_HDP
/* the NanoporeHDP as densities need it (dir_proc_density impl/hdp.c:2577-2601 -> grid_spline_interp
 * impl/hdp_math_utils.c:471-495): an evenly spaced sampling grid, values and spline slopes per table row */
struct HdpGrid {
    const double *__restrict__ grid, *__restrict__ y, *__restrict__ slope;
    int n;              /* index of the grid's last point */
    double x0, xn, dx;  /* its first and last point, its spacing */
};
__device__ __forceinline__ HdpGrid hdp_grid(const double *model) {
    const DevHdpModel *hm = (const DevHdpModel *) model;
    HdpGrid h;
    h.grid = hm->grid; h.y = hm->y; h.slope = hm->slope;
    h.n = uni(hm->gridLength) - 1;
    h.x0 = h.grid[0]; h.xn = h.grid[h.n]; h.dx = h.grid[1] - h.grid[0];
    return h;
}
/* (grid cell, offset in it) of an event's mean, as grid_spline_interp takes them -- its two IEEE divisions, once per
 * event; -1 / -2 with the distance to the grid's end for a mean below / above the grid (cpecan_k_wv_forward_h*) */
__device__ __forceinline__ void hdp_event(const HdpGrid &h, double q, double &cell, double &off) {
    if (q <= h.x0) { cell = -1.0; off = h.x0 - q; }
    else if (q >= h.xn) { cell = -2.0; off = q - h.xn; }
    else {
        const long long il = (long long) ((q - h.x0) / h.dx);
        cell = (double) il;
        off = (q - h.grid[il]) / h.dx;
    }
}
#endif

#ifdef SY_VANILLA
/* emissions_signal_getEventMatchProbWithTwoDists (impl/stateMachine.c:499-528) on one table of a slot's row (p: mu, sd,
 * 1/sd, K, noise mean, 1/mean, lambda, log(lambda) - log(2 pi)): logGaussPdf of the event's mean (:333-343) plus
 * logInvGaussPdf of its noise (:322-331), ((log(lambda) - log(2 pi) - 3 log(noise)) - lambda a a / noise) / 2 with
 * a = (noise - mu) / mu.  Both divisions are Markstein-corrected multiplies (by the track's 1/mu and by the 1/noise
 * taken when the event was staged), log(noise) is the host's: the same doubles as the wave builds' and the oracle's. */
__device__ __forceinline__ double vemit(double em, double en, double er, double c3, const double *p) {
    const double level = lgauss(em, p[0], p[1], p[2], p[3]);
    const double u = en - p[4];
    const double q1 = u * p[5];
    const double a = __fma_rn(__fma_rn(-q1, p[4], u), p[5], q1); /* (noise - mu) / mu */
    const double w = p[6] * a * a;
    const double q2 = w * er;
    const double dv = __fma_rn(__fma_rn(-q2, en, w), er, q2);    /* lambda a a / noise */
    return level + (p[7] - c3 - dv) / 2;
}

/* The sweep back keeps a slot's five log transition probabilities; those of the k-mers that enter at the band's low edge
 * come from an LDS ring by k-mer index, which the whole workgroup refills from the track every 32 diagonals (k-mers
 * enter in descending order, at most one per diagonal) */
#define SY_TR_RING 128
#define SY_TR_AHEAD 119 /* staged below the next k-mer to enter; the eight entries above it are left alone, a wave one
                         * step behind may still be reading the last one */
struct TransFeed {
    double r[SY_TR_RING * 5];
};
/* k-mers lo..hi (0 <= lo) into the ring; the whole workgroup */
__device__ __forceinline__ void trans_stage(TransFeed &tf, const double *__restrict__ track, int lo, int hi) {
    for (int i = lo * 5 + (int) threadIdx.x; i < (hi + 1) * 5; i += SY_P) {
        const int x = i / 5, j = i - x * 5;
        tf.r[(x & (SY_TR_RING - 1)) * 5 + j] = track[(long long) x * SY_ROW + SY_TR + j];
    }
}
#endif

/*
 * The band: first and last matrix column (k-mer index) of every anti-diagonal, one int2 per diagonal
 * in HBM, built by the host from band_construct's output (cpecan_hip.hip).  The sweeps read it
 * through a 128-entry LDS ring that the whole workgroup refills every 32 diagonals, so a step costs
 * one LDS read instead of walking the anchor rectangles on the scalar unit.
 */
#define SY_BAND_RING 128
struct BandFeed {
    int2 e[SY_BAND_RING];
};
/* entries of diagonals lo..hi (clipped to 0..D) into the ring; the whole workgroup */
__device__ __forceinline__ void band_stage(BandFeed &bf, const int2 *__restrict__ tab, int D, int lo, int hi) {
    for (int d = lo + (int) threadIdx.x; d <= hi; d += SY_P)
        if (d >= 0 && d <= D) bf.e[d & (SY_BAND_RING - 1)] = tab[d];
}
__device__ __forceinline__ void band_get(const BandFeed &bf, int d, int &xmin, int &xmax) {
    const int2 v = bf.e[d & (SY_BAND_RING - 1)];
    xmin = uni(v.x);
    xmax = uni(v.y);
}
/* straight from HBM (start-up paths only) */
__device__ __forceinline__ void band_load(const int2 *__restrict__ tab, int d, int &xmin, int &xmax) {
    const int2 v = tab[d > 0 ? d : 0];
    xmin = uni(v.x);
    xmax = uni(v.y);
}

/* does wave w hold an in-band slot: waves (xmin>>6) .. (xmax>>6), modulo R */
__device__ __forceinline__ bool row_active(int w, int xmin, int xmax) {
    int first = xmin >> 6, n = (xmax >> 6) - first;
    return SY_WMOD(w - first) <= n;
}

/* logAdd-fold of one value per lane into acc (wave-uniform in and out), lanes in ascending order;
 * visits only the lanes that can change the running value (cp_wave_seq_fold with the LDS-table
 * logAdd, so that no coefficient constants occupy registers around the call) */
__device__ __forceinline__ double wave_fold(double acc, double v, const double *coef) {
    const int lane = threadIdx.x & 63;
    unsigned long long after = ~0ull;
#pragma unroll 1
    for (;;) {
        const bool eff = ((after >> lane) & 1ull) && (v > CP_NEG_INF) && !(acc - v >= 7.5);
        const unsigned long long m = __ballot(eff);
        if (m == 0ull) break;
        const int first = __ffsll((long long) m) - 1;
        acc = ladd(acc, bcast(v, first), coef);
        after = first >= 63 ? 0ull : (~0ull << (first + 1));
    }
    return acc;
}

__device__ __forceinline__ void load_params(double (&dst)[SY_NPRM], const double *__restrict__ track, int x) {
    const double *p = track + (long long) x * SY_ROW;
#pragma unroll
    for (int j = 0; j < SY_NPRM; j++) dst[j] = p[j];
}
__device__ __forceinline__ double set_lane(double v, int dst, double x) { /* x, dst wave-uniform */
    if ((int) (threadIdx.x & 63) == dst) v = x;
    return v;
}

/* lane i <- lane i-1 of src, lane 0 <- old (DPP wave_shr:1 leaves lanes without a source untouched) */
__device__ __forceinline__ double shr1(double old, double src) {
    int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), 0x138, 0xf, 0xf, false);
    int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), 0x138, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}
/* lane i <- lane i+1 of src, lane 63 <- old */
__device__ __forceinline__ double shl1(double old, double src) {
    int lo = __builtin_amdgcn_update_dpp(__double2loint(old), __double2loint(src), 0x130, 0xf, 0xf, false);
    int hi = __builtin_amdgcn_update_dpp(__double2hiint(old), __double2hiint(src), 0x130, 0xf, 0xf, false);
    return __hiloint2double(hi, lo);
}

struct Geometry {
    int lane, wave, waveBelow, waveAbove;
    double *rw, *rwb; /* ring bases of this lane's slot and of the slot below it */
    int ringMask;
    __device__ __forceinline__ double *rp(int d, int s) const {
        return rw + (long long) (d & ringMask) * (SY_R * SY_RING_VALUES * 64) + s * 64;
    }
    __device__ __forceinline__ double *rpb(int d, int s) const {
        return rwb + (long long) (d & ringMask) * (SY_R * SY_RING_VALUES * 64) + s * 64;
    }
};

__device__ __forceinline__ Geometry make_geometry(double *ring, int ringD) {
    Geometry g;
    g.lane = threadIdx.x & 63;
    g.wave = uni(threadIdx.x >> 6);
    g.waveBelow = (g.wave + SY_R - 1) % SY_R;
    g.waveAbove = (g.wave + 1) % SY_R;
    /* ring of forward diagonals: [diagonal & (ringD-1)][wave][Fm,Fx,Fy,pm,py][lane] */
    g.rw = ring + g.wave * (SY_RING_VALUES * 64) + g.lane;
    g.rwb = ring + (g.lane == 0 ? g.waveBelow : g.wave) * (SY_RING_VALUES * 64) + ((g.lane + 63) & 63);
    g.ringMask = ringD - 1;
    return g;
}

/* The next traceback point (:917-921) from the band alone: the first diagonal above dAfter that is at
 * least dMin and narrow enough, or the last diagonal D.  Whole workgroup, SY_P diagonals per round. */
__device__ int next_traceback_point(const int2 *__restrict__ tab, int D, int dAfter, long long dMin,
                                    long long widthLimit, Shared &sh) {
    long long b0 = dAfter + 1 > dMin ? dAfter + 1 : dMin;
    if (b0 >= D) return D;
    int base = (int) b0;
    for (;;) {
        __syncthreads();
        if (threadIdx.x == 0) sh.item = 0x7fffffff;
        __syncthreads();
        const int d = base + (int) threadIdx.x;
        if (d >= D) atomicMin(&sh.item, D);
        else {
            const int2 v = tab[d];
            if ((long long) (v.y - v.x + 1) <= widthLimit) atomicMin(&sh.item, d);
        }
        __syncthreads();
        const int r = uni(sh.item);
        if (r != 0x7fffffff) return r;
        base += SY_P;
    }
}

/* Forward sweep of one alignment from its saved diagonal up to (and including) the next traceback
 * point; describes the window for the backward kernel. */
__device__ void forward_window(const DevItem &it, const DevParams &P, const int2 *__restrict__ bandTab,
                               const double *__restrict__ track, const double *__restrict__ events,
                               const double *__restrict__ model, double *ring, int ringD,
                               SyState *state, Shared &sh, Feed &fd, BandFeed &bf) {
    const Geometry g = make_geometry(ring, ringD);
    const int lane = g.lane, wave = g.wave;
    const int lX = (int) it.lX, lY = (int) it.lY, D = lX + lY;
    const double *__restrict__ ev = events + 3 * it.yOff;
    const double *cf = sh.coef;
#ifdef SY_VANILLA
    /* the position-independent transitions (cpecan_models.hip: derive_vanilla); the others are the slot row's */
    const double lYM = model[CP_VHDR_LOG_YM], lYY = model[CP_VHDR_LOG_YY];
#else
    /* a -inf gapY->gapX transition (the nanopore default, stateMachine.c:1287) contributes
     * logAdd(acc, -inf) == acc: skip that term (wave-uniform) */
    const bool hasSwitchX = model[T_GAP_SWITCH_TO_X] > CP_NEG_INF;
    double T[9];
#pragma unroll
    for (int i = 0; i < 9; i++) T[i] = model[i];
#endif
#ifdef SY_HDP
    const HdpGrid hg = hdp_grid(model);
#endif

    const int d0 = uni(ld_agent(&state->d));
    int tracedBackTo = uni(ld_agent(&state->tracedBackTo));
    long long cells = uni64(ld_agent(&state->cells));

    /* ---- per-slot state (this lane's k-mer) ---- */
    int xs;
    double prm[SY_NPRM];
    double Fm, Fx, Fy; /* forward cell, current diagonal   */
    double Lm, Lx, Ly; /* slot-1's cell, previous diagonal */
    double em, en;     /* event scored on this diagonal    */
#ifdef SY_VANILLA
    double er, el;     /* ... its 1 / noise and log(noise); an event that does not exist is (0, 1, 1, 0): finite */
#endif
    int xin, xminP;

    if (d0 == 0) {
        /* diagonal 0: the single cell (0,0) holds the start vector (:897-898, stateMachine.c:1168-1177) */
        xs = wave * 64 + lane;
#pragma unroll
        for (int j = 0; j < SY_NPRM; j++) prm[j] = 0.0;
#ifdef SY_HDP
        prm[0] = -1.0; /* no k-mer yet: a parked slot scores -inf */
#endif
        Fm = Fx = Fy = Lm = Lx = Ly = CP_NEG_INF;
#ifdef SY_VANILLA
        em = el = 0.0;
        en = er = 1.0;
#else
        em = en = 0.0;
#endif
        if (wave == 0 && lane == 0) {
            load_params(prm, track, 0);
            Fm = it.raggedL ? CP_NEG_INF : 0.0;
            Fx = it.raggedL ? 0.0 : CP_NEG_INF;
            Fy = Fx;
        }
        if (wave == 0 && lane == 0) { /* only cells of the band are ever stored to the ring */
            *g.rp(0, 0) = Fm;
            *g.rp(0, 1) = Fx;
            *g.rp(0, 2) = Fy;
            *g.rp(0, 3) = 0.0;
            *g.rp(0, 4) = 0.0;
        }
        cells += 1;
        xin = 1;
        xminP = 0;
    } else {
        /* resume at d0: constants of the k-mers in the band, forward cells of d0 and d0-1, events */
        int xmin, xmax, qmin, qmax;
        band_load(bandTab, d0 - 1, qmin, qmax);
        band_load(bandTab, d0, xmin, xmax);
        xs = wave * 64 + lane;
        xs += ((xmin - xs + SY_P - 1) / SY_P) * SY_P; /* the k-mer >= xmin that lives in this slot */
        const bool v = xs <= xmax;
        load_params(prm, track, xs <= lX ? xs : lX);
        /* ring slots of cells outside the band hold stale data: mask per lane */
        Fm = v ? *g.rp(d0, 0) : CP_NEG_INF;
        Fx = v ? *g.rp(d0, 1) : CP_NEG_INF;
        Fy = v ? *g.rp(d0, 2) : CP_NEG_INF;
        const bool a1 = xs - 1 >= qmin && xs - 1 <= qmax;
        Lm = a1 ? *g.rpb(d0 - 1, 0) : CP_NEG_INF;
        Lx = a1 ? *g.rpb(d0 - 1, 1) : CP_NEG_INF;
        Ly = a1 ? *g.rpb(d0 - 1, 2) : CP_NEG_INF;
        const int ei = d0 - xs - 1;
        const bool okE = v && ei >= 0 && ei < lY;
        em = okE ? ev[3 * (long long) ei] : 0.0;
#ifdef SY_HDP
        en = 0.0;
        if (okE) hdp_event(hg, em, em, en);
#elif defined(SY_VANILLA)
        en = okE ? ev[3 * (long long) ei + 1] : 1.0;
        er = okE ? 1.0 / en : 1.0;
        el = okE ? ev[3 * (long long) ei + 2] : 0.0;
#else
        en = okE ? ev[3 * (long long) ei + 1] : 0.0;
#endif
        xin = xmax + 1;
        xminP = xmin;
    }
    int evHi = d0 - xminP - 1, rowHi = xin; /* first event / k-mer row not yet staged */

    /*
     * Which diagonals need all three states in the ring.  The sweep back reads only the match cell of
     * a diagonal, except where it refreshes totalProbability (every 10th decoded diagonal, counted
     * down from the first one of ITS window: it then reads every state of that diagonal and of the
     * one below), and this sweep resumes from the last two diagonals of a launch.  Where the windows
     * will start is a function of the band alone, so it is known here: this launch ends at topW; its
     * diagonals up to fromW are decoded by window W (first decoded diagonal tpA), the ones above by
     * the next window (tpB).  Everywhere else the two gap states are not stored: 16 of the 40 bytes
     * a cell costs on the way up.
     */
    const long long widthLimit = P.expansion * 2 + 1;
    const int topW = next_traceback_point(bandTab, D, d0, tracedBackTo + P.minDiags, widthLimit, sh);
    const bool endW = topW == D;
    const int fromW = topW - (endW ? 0 : (int) P.tbDiags + 1);
    const int tpA = topW < fromW ? topW : fromW;
    int tpB = tpA;
    bool allFull = false;
    if (!endW) {
        const int topN = next_traceback_point(bandTab, D, topW, fromW + P.minDiags, widthLimit, sh);
        const int fromN = topN - (topN == D ? 0 : (int) P.tbDiags + 1);
        tpB = topN < fromN ? topN : fromN;
        allFull = tpB < topW; /* windows shorter than the traceback margin: keep everything */
    }
    if (SY_MODE(P) != 0) allFull = true; /* the expectation pass reads every state of every diagonal */
    /* (tpA - d) mod 10 and (tpB - d) mod 10 for the diagonal being computed, kept incrementally */
    /* (tpA - d) mod 10 and (tpB - d) mod 10 for the next diagonal whose mask bit is computed */
    int rA = ((tpA - (d0 + 1)) % 10 + 10) % 10, rB = endW ? 0x40000000 : ((tpB - (d0 + 1)) % 10 + 10) % 10;
    const int fullFrom = allFull ? -0x40000000 : topW - 1;
    if (lane == 63) {
        double *x = sh.xch[d0 & 1][wave];
        x[0] = Fm; x[1] = Fx; x[2] = Fy; x[3] = em; x[4] = en;
#ifdef SY_VANILLA
        x[5] = er; x[6] = el;
#endif
    }

    const long long tbFromL = tracedBackTo + P.minDiags;
    const int tbFrom = uni((int) (tbFromL < 0x7fffffff ? tbFromL : 0x7fffffff));
    const int tbWidth = uni((int) (widthLimit < 0x7fffffff ? widthLimit : 0x7fffffff));
    PROF_DECL
    /* blocks of SY_FEED diagonals: the loads sit between the blocks, the inner loop has none (but for the -DSY_HDP
     * build's four table values per cell, see its emission below) */
#pragma unroll 1
    for (int db = d0 + 1; db <= D; db += SY_FEED) {
        {
            /* stage what the next two blocks of diagonals can ask for: the top cell's event index
             * d-xmin-1 and the entering k-mer xin each advance by at most one per diagonal */
            int fxmin, fxmax;
            band_load(bandTab, db, fxmin, fxmax);
            band_stage(bf, bandTab, D, db, db + 2 * SY_FEED - 1);
            const int evTo = db - fxmin - 1 + 3 * SY_FEED, rowTo = xin + 2 * SY_FEED;
#ifdef SY_VANILLA
#pragma unroll 1
            for (int i = evHi * SY_EVW + (int) threadIdx.x; i < evTo * SY_EVW; i += SY_P) {
                /* 1 / noise is taken once, here; log(noise) is the host's (the batch's own copy of the events carries it
                 * in place of the duration) */
                const int e = i >> 2, c = i & 3;
                const bool ok = e >= 0 && e < lY;
                const double q = ok ? ev[3 * (long long) e + (c == 0 ? 0 : c == 3 ? 2 : 1)] : (c == 0 || c == 3 ? 0.0 : 1.0);
                fd.ev[(i & (SY_EVW * SY_FEED_EV - 1))] = c == 2 ? 1.0 / q : q;
            }
#elif defined(SY_HDP)
#pragma unroll 1
            for (int e = evHi + (int) threadIdx.x; e < evTo; e += SY_P) {
                /* an event that does not exist stays at (0, 0): it only ever meets -inf cells and must score
                 * something finite */
                double c = 0.0, o = 0.0;
                if (e >= 0 && e < lY) hdp_event(hg, ev[3 * (long long) e], c, o);
                fd.ev[(2 * e) & (2 * SY_FEED_EV - 1)] = c;
                fd.ev[(2 * e + 1) & (2 * SY_FEED_EV - 1)] = o;
            }
#else
#pragma unroll 1
            for (int i = evHi * 2 + (int) threadIdx.x; i < evTo * 2; i += SY_P) {
                const int e = i >> 1;
                fd.ev[(i & (2 * SY_FEED_EV - 1))] = e >= 0 && e < lY ? ev[3 * (long long) e + (i & 1)] : 0.0;
            }
#endif
#pragma unroll 1
            for (int i = rowHi * SY_FEEDW + (int) threadIdx.x; i < rowTo * SY_FEEDW; i += SY_P) {
                const int x = i / SY_FEEDW, j = i - x * SY_FEEDW;
                fd.row[(x & (SY_FEED_ROW - 1)) * SY_FEEDW + j] = track[(long long) (x <= lX ? x : lX) * SY_ROW + j];
            }
            evHi = evTo;
            rowHi = rowTo;
            __builtin_amdgcn_s_waitcnt(0x0F70); /* vmcnt(0): nothing pending past this point */
        }
        const int dbEnd = db + SY_FEED - 1 < D ? db + SY_FEED - 1 : D;
        unsigned fullMask = 0u; /* bit j: diagonal db + j keeps all three states */
#pragma unroll 1
        for (int j = 0; j < SY_FEED; j++) {
            const int dj = db + j;
            const int rHere = dj <= fromW ? rA : rB, rAbove = dj + 1 <= fromW ? rA : rB;
            fullMask |= (dj >= fullFrom || rHere == 0 || rAbove == 1 ? 1u : 0u) << j;
            rA = rA == 0 ? 9 : rA - 1;
            rB = rB == 0 ? 9 : rB - 1;
        }
        fullMask = (unsigned) uni((int) fullMask);
#pragma unroll 1
        for (int d = db; d <= dbEnd; d++) {
        PROF(0)
        PROF(1)
        lds_barrier(); /* also orders the band/event/k-mer staging above before the reads below */
        int xmin, xmax;
#ifdef SY_ABLATE_BAND
        xmin = d / 3; xmax = xmin + 132;
#else
        band_get(bf, d, xmin, xmax);
#endif
        cells += xmax - xmin + 1;
        const bool full = ((fullMask >> (d - db)) & 1u) != 0u;
        PROF_ACTIVE(row_active(wave, xmin, xmax))
        PROF(2)
#ifdef SY_ABLATE_XCH
        const double rm = shr1(Fm, Fm), rx = shr1(Fx, Fx), ry = shr1(Fy, Fy);
        em = shr1(em, em);
        en = shr1(en, en);
#else
        const double *xb = sh.xch[(d - 1) & 1][g.waveBelow];
        const double rm = shr1(xb[0], Fm), rx = shr1(xb[1], Fx), ry = shr1(xb[2], Fy);
        em = shr1(xb[3], em);
        en = shr1(xb[4], en);
#ifdef SY_VANILLA
        er = shr1(xb[5], er);
        el = shr1(xb[6], el);
#endif
#endif
        PROF_FENCE(em) PROF_FENCE(en)
        PROF(3)
        if (xs < xmin) xs += SY_P;
        const bool valid = xs <= xmax;
        while (xin <= xmax) { /* the entering k-mer's constants (at most one k-mer per step) */
#ifdef SY_ABLATE_INSTALL
            if (d == -1) {
#else
            if (SY_WAVE_OF(xin) == wave && lane == (xin & 63)) {
#endif
                const double *r = fd.row + (xin & (SY_FEED_ROW - 1)) * SY_FEEDW;
#pragma unroll
                for (int j = 0; j < SY_NPRM; j++) prm[j] = r[j];
            }
            xin++;
        }
        if (xmin == xminP && SY_WAVE_OF(xmin) == wave && lane == (xmin & 63)) {
            /* the top cell's event is new.  Index -1 is NULLEVENT (:261): its emissions only ever
             * meet -inf cells, the staged 0.0 keeps NaN out */
            const double *e = fd.ev + ((SY_EVW * (d - xmin - 1)) & (SY_EVW * SY_FEED_EV - 1));
            em = e[0];
            en = e[1];
#ifdef SY_VANILLA
            er = e[2];
            el = e[3];
#endif
        }
        PROF_FENCE(em) PROF_FENCE(en) PROF_FENCE(prm[0])
        PROF(4)
        double nmv = CP_NEG_INF, nxv = CP_NEG_INF, nyv = CP_NEG_INF;
        if (row_active(wave, xmin, xmax)) {
#ifdef SY_VANILLA
            const double c3 = 3 * el;
            const double pm = vemit(em, en, er, c3, prm), py = vemit(em, en, er, c3, prm + 8);
            /* cell_calculateForward over stateMachine3Vanilla_cellCalculate (stateMachine.c:1368-1409): gap X from the
             * lower cell (no emission: 0 + tP is tP), match from the middle cell, gap Y from the upper cell */
            double gx = rm + prm[SY_TR + 0];
            gx = ladd(gx, rx + prm[SY_TR + 1], cf);
            double mm = Lm + (pm + prm[SY_TR + 2]);
            mm = ladd(mm, Lx + (pm + prm[SY_TR + 3]), cf);
            mm = ladd(mm, Ly + (pm + lYM), cf);
            double gy = Fm + (py + prm[SY_TR + 4]);
            gy = ladd(gy, Fy + (py + lYY), cf);
#else
#ifdef SY_HDP
            /* get_nanopore_kmer_density (impl/nanopore_hdp.c:390): the spline of the slot's table row at the cell's
             * event, clamped at zero -- a linear density where a log-probability belongs, match and gap-Y emission
             * alike; a column that is no k-mer (row offset < 0) scores -inf.  Four values of the model's tables per
             * cell: the only global loads of the sweep (the tables stay in L2). */
            const double px = SY_HDP_GAPX;
            double pm, py;
            {
                const double ro = prm[0], ex = em, w = en;
                /* (32-bit indices: cpecan_hip_modelsh_create refuses tables of 2^32 values or more) */
                const unsigned base = ro < 0.0 ? 0u : (unsigned) ro;
                const unsigned il = ex < 0.0 ? (ex == -2.0 ? (unsigned) hg.n : 0u) : (unsigned) ex;
                const unsigned ir = ex < 0.0 ? il : il + 1u;
                const double yl = hg.y[base + il], yr = hg.y[base + ir];
                const double sl = hg.slope[base + il], sr = hg.slope[base + ir];
                const double dy = yr - yl;
                const double ca = sl * hg.dx - dy, cb = dy - sr * hg.dx;
                const double tl = w, tr = 1.0 - tl;
                const double inside = tr * yl + tl * yr + tl * tr * (ca * tr + cb * tl);
                const double edge = ex == -1.0 ? yl - sl * w : yl + sl * w;
                double r = ex < 0.0 ? edge : inside;
                r = r > 0.0 ? r : 0.0;
                pm = py = ro < 0.0 ? CP_NEG_INF : r;
            }
#else
            const double px = prm[CP_GAPX];
#ifdef SY_ABLATE_EMIT
            double pm = em + prm[CP_K1], py = en + prm[CP_YK1];
#else
            double pm = lgauss(em, prm[CP_MU], prm[CP_SD], prm[CP_RSD], prm[CP_K1])
                            + lgauss(en, prm[CP_NMU], prm[CP_NSD], prm[CP_RNSD], prm[CP_K2]);
            double py = lgauss(em, prm[CP_YMU], prm[CP_YSD], prm[CP_RYSD], prm[CP_YK1])
                            + lgauss(en, prm[CP_YNMU], prm[CP_YNSD], prm[CP_RYNSD], prm[CP_YK2]);
#endif
#endif /* SY_HDP */
            PROF_FENCE(pm) PROF_FENCE(py)
            PROF(5)
            /* cell_calculateForward: to[t] = logAdd(to[t], from[f] + (eP + tP)) (:365-376) in the
             * order of stateMachine3_cellCalculate (stateMachine.c:1314-1333) */
            double gx = rm + (px + T[T_GAP_OPEN_X]);
            gx = ladd(gx, rx + (px + T[T_GAP_EXTEND_X]), cf);
            if (hasSwitchX) gx = ladd(gx, ry + (px + T[T_GAP_SWITCH_TO_X]), cf);
            double mm = Lm + (pm + T[T_MATCH_CONTINUE]);
            mm = ladd(mm, Lx + (pm + T[T_MATCH_FROM_GAP_X]), cf);
            mm = ladd(mm, Ly + (pm + T[T_MATCH_FROM_GAP_Y]), cf);
            double gy = Fm + (py + T[T_GAP_OPEN_Y]);
            gy = ladd(gy, Fy + (py + T[T_GAP_EXTEND_Y]), cf);
#endif /* SY_VANILLA */
            PROF_FENCE(mm) PROF_FENCE(gx) PROF_FENCE(gy)
            PROF(6)
            nmv = valid ? mm : CP_NEG_INF;
            nxv = valid ? gx : CP_NEG_INF;
            nyv = valid ? gy : CP_NEG_INF;
#ifdef SY_ABLATE_STORE
            if (valid && d == -1) {
#else
            if (valid) { /* cells outside the band cost no HBM traffic */
#endif
                *g.rp(d, 0) = mm;
                if (full) {
                    *g.rp(d, 1) = gx;
                    *g.rp(d, 2) = gy;
                }
                *g.rp(d, 3) = pm; /* the sweep back re-uses the two event-dependent emissions */
                *g.rp(d, 4) = py;
            }
        }
        PROF(7)
        Lm = rm; Lx = rx; Ly = ry;
        Fm = nmv; Fx = nxv; Fy = nyv;
        if (lane == 63) {
            double *x = sh.xch[d & 1][wave];
            x[0] = Fm; x[1] = Fx; x[2] = Fy; x[3] = em; x[4] = en;
#ifdef SY_VANILLA
            x[5] = er; x[6] = el;
#endif
        }
        xminP = xmin;
        PROF(8)

        const bool atEnd = d == D;
        const bool tb = d >= tbFrom && xmax - xmin < tbWidth; /* both wave-uniform 32-bit: scalar compares */
        if (atEnd || tb) { /* traceback point (:917-921): hand the window to the backward kernel */
            if (threadIdx.x == 0) {
                const int from = d - (atEnd ? 0 : (int) P.tbDiags + 1);
                state->d = d;
                state->finished = atEnd ? 1 : 0;
                state->winValid = 1;
                state->winTop = d;
                state->winFrom = from;
                state->winTo = tracedBackTo;
                state->winAtEnd = atEnd ? 1 : 0;
                state->tracedBackTo = from;
                state->cells = cells;
            }
            PROF_FLUSH(wave)
            return;
        }
        }
    }
}

#ifdef SY_FUSED
__device__ __forceinline__ double uni_d(double v) {
    return __hiloint2double(uni(__double2hiint(v)), uni(__double2loint(v)));
}

/*
 * Fused Baum-Welch expectations (-DSY_FUSED): what the sweep back leaves per refresh segment of a window (the ten decoded
 * diagonals that share one totalProbability), in the alignment's HBM scratch behind what sy_scratch_bytes counts:
 *   tr  the eight transition sums of every wave, [segment][wave][8]
 *   g   per slot two gap-X sums, [segment][A | B][slot]: B the sum of the slot's column at the segment's end, A that of
 *       the column it held before, when the slot changed columns within the segment.  One change at most: a slot's
 *       column steps by SY_P >= 64 and a band edge moves by at most one column per diagonal, so a second change would
 *       need the band to travel SY_P columns within the segment's eleven diagonals
 *   c   their matrix columns (-1: none)
 * The sweep writes every record of every segment it closes, so nothing is left over from an earlier window or run.
 * The vanilla machine (-DSY_VANILLA) collects two sums per cell and no transition: no tr, and a record of g is the pair
 * (beta: match -> gap X, alpha: gap X -> gap X) of its column, [segment][A | B][slot][2].
 */
struct FxRecords {
    double *tr, *g;
    int *c;
};
#ifdef SY_VANILLA
#define SY_FX_TR 0 /* doubles per wave and segment of tr, per record of g */
#define SY_FX_G 2
#elif defined(SY_HDP)
#define SY_FX_TR 8
#define SY_FX_G 0 /* the HDP machine collects no gap-X sums per k-mer: no g and no c */
#else
#define SY_FX_TR 8
#define SY_FX_G 1
#endif
static __host__ __device__ long long sy_fx_bytes(int ringD) {
    return ((long long) ringD / 10 + 8)
           * (SY_R * SY_FX_TR * sizeof(double) + 2 * SY_P * (SY_FX_G ? SY_FX_G * sizeof(double) + sizeof(int) : 0));
}
__device__ __forceinline__ FxRecords fx_records(char *base, int ringD) {
    const long long nW = (long long) ringD / 10 + 8;
    FxRecords f;
    f.tr = (double *) base;
    f.g = f.tr + nW * SY_R * SY_FX_TR;
    f.c = (int *) (f.g + nW * 2 * SY_P * SY_FX_G);
    return f;
}
#ifdef SY_VANILLA
/* A window's fused sums into the model's expectations (layout of cpecan_k_sy_expect's, vanilla form: 30 + 30 skip bins and
 * the likelihood); the whole workgroup.  Segment k's sums were taken against the estimate and scale by
 * exp(est - total_k), or, on the second sweep (exact), against total_k itself.  Every thread adds the records of its
 * slot, one pair of LDS atomics per column, to the window's 60 bin sums (bins: SY_P doubles of LDS no E-step uses
 * otherwise), the bin being entry 21 of the column's track row; then threads 0-59 add those to the model's, thread 60 the
 * likelihood (the exact total once per decoded diagonal, :849). */
__device__ void fx_finish(const DevItem &it, const FxRecords &fx, const WinTotal *wtot, const int nSeg, const int tPost0,
                          const int to, const double est, const bool exact, double *expect,
                          const double *__restrict__ track, double *bins) {
    double *dst = expect + (long long) it.model * CP_EXPECTV_LEN;
    const int tid = threadIdx.x;
    if (tid < 60) bins[tid] = 0.0;
    __syncthreads();
    auto add = [&](const int col, const double beta, const double alpha) __attribute__((always_inline)) {
        const int bin = col > 0 && col <= (int) it.lX ? (int) track[(long long) col * SY_ROW + 21] : -1;
        if (bin >= 0 && bin < 30) {
            if (beta != 0.0) atomicAdd(&bins[bin], beta);
            if (alpha != 0.0) atomicAdd(&bins[bin + 30], alpha);
        }
    };
    int cur = -1;
    double beta = 0.0, alpha = 0.0;
#pragma unroll 1
    for (int k = 0; k < nSeg; k++) {
        const double f = exact ? 1.0 : exp(est - wtot[k].total);
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const long long i = (long long) (k * 2 + r) * SY_P + tid;
            const int col = fx.c[i];
            const double b = fx.g[i * 2], a = fx.g[i * 2 + 1];
            if (col > 0 && (b != 0.0 || a != 0.0)) {
                if (col != cur) {
                    add(cur, beta, alpha);
                    cur = col;
                    beta = alpha = 0.0;
                }
                beta += f * b;
                alpha += f * a;
            }
        }
    }
    add(cur, beta, alpha);
    __syncthreads();
    if (tid < 60) {
        if (bins[tid] != 0.0) atomicAdd(dst + tid, bins[tid]);
    } else if (tid == 60) {
        double lik = 0.0;
#pragma unroll 1
        for (int u = tPost0; u > to; u--) lik += wtot[(tPost0 - u) / 10].total;
        atomicAdd(dst + 60, lik);
    }
}
#else
/* M>X X>X Y>X | M>M X>M Y>M | M>Y Y>Y into the model's nine transition sums (from * 3 + to) */
#define SY_EXPECT_SLOTS { 0 * 3 + 1, 1 * 3 + 1, 2 * 3 + 1, 0 * 3 + 0, 1 * 3 + 0, 2 * 3 + 0, 0 * 3 + 2, 2 * 3 + 2 }
#ifdef SY_HDP
#define SY_FX_LIK 9 /* the likelihood follows the nine transitions */
#define SY_FX_LEN (9 + 1) /* CPECAN_EXPECTATIONH_LEN doubles per model */
#else
#define SY_FX_LIK (9 + 4096) /* ... the 4096 k-mer bins */
#define SY_FX_LEN (9 + 4096 + 1)
#endif

/* A window's fused sums into the model's expectations (layout of cpecan_k_sy_expect's); the whole workgroup.  Segment
 * k's sums were taken against the estimate and scale by exp(est - total_k), or, on the second sweep (exact), against
 * total_k itself.  Threads 0-7 the transitions, thread 8 the likelihood (the exact total once per decoded diagonal,
 * :849), every thread the gap-X sums of its slot, one atomic per column, into the bins of the columns' k-mers. */
__device__ void fx_finish(const DevItem &it, const FxRecords &fx, const WinTotal *wtot, const int nSeg, const int tPost0,
                          const int to, const double est, const bool exact, double *expect,
                          const unsigned short *__restrict__ kidx) {
    double *dst = expect + (long long) it.model * SY_FX_LEN;
    const int slot[8] = SY_EXPECT_SLOTS;
    const int tid = threadIdx.x;
    if (tid < 8) {
        double sum = 0.0;
#pragma unroll 1
        for (int k = 0; k < nSeg; k++) {
            double seg = 0.0;
            for (int w = 0; w < SY_R; w++) seg += fx.tr[(k * SY_R + w) * 8 + tid];
            sum += seg * (exact ? 1.0 : exp(est - wtot[k].total));
        }
        atomicAdd(dst + slot[tid], sum);
    } else if (tid == 8) {
        double lik = 0.0;
#pragma unroll 1
        for (int u = tPost0; u > to; u--) lik += wtot[(tPost0 - u) / 10].total;
        atomicAdd(dst + SY_FX_LIK, lik);
    }
#ifdef SY_HDP /* (no k-mer bins) */
    (void) kidx;
#else
    const unsigned short *kx = kidx + it.xOff;
    int cur = -1;
    double sum = 0.0;
#pragma unroll 1
    for (int k = 0; k < nSeg; k++) {
        const double f = exact ? 1.0 : exp(est - wtot[k].total);
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int col = fx.c[(k * 2 + r) * SY_P + tid];
            const double v = fx.g[(k * 2 + r) * SY_P + tid];
            if (col > 0 && v != 0.0) {
                if (col != cur) {
                    if (cur > 0 && kx[cur - 1] < 4096) atomicAdd(dst + 9 + kx[cur - 1], sum);
                    cur = col;
                    sum = 0.0;
                }
                sum += f * v;
            }
        }
    }
    if (cur > 0 && kx[cur - 1] < 4096) atomicAdd(dst + 9 + kx[cur - 1], sum);
#endif
}
#endif /* SY_VANILLA */
#endif /* SY_FUSED */

/*
 * Backward sweep + posterior decode of one traceback window (:921-992), in three phases:
 *  S  the sweep back: one anti-diagonal per iteration, cells and messages in registers.  It leaves
 *     per cell F.match + B.match (in the ring slot of the match emission, dead by then) and, on the
 *     diagonals where the reference refreshes totalProbability, the two per-cell terms of that sum
 *     (HBM scratch);
 *  T  totalProbability (:736-754) for every refresh of the window at once: the reference's
 *     order-dependent logAdd fold is inherently serial, so each THREAD folds one diagonal's terms
 *     privately, in the reference's order -- ~200 independent chains instead of one wave-wide chain
 *     per refresh inside the sweep;
 *  D  diagonalCalculationPosteriorMatchProbs (:756-795) for the window: hits are counted per
 *     diagonal, prefix-summed in emission order (diagonals descending, x-y ascending) and written.
 */
__device__ void backward_window(const DevItem &it, const DevParams &P, const int2 *__restrict__ bandTab,
                                const double *__restrict__ track, const double *__restrict__ model,
                                double *ring, int ringD, SyState *state, ItemOut &out, Shared &sh,
                                BandFeed &bf, int *cntBuf, WinTotal *wtot, double *vw,
                                unsigned long long *msk, int2 *candKx, double *candFb, double *bring
#ifdef SY_VANILLA
                                , TransFeed &tf
#endif
#ifdef SY_FUSED
                                , const FxRecords &fxo, double *expect, const unsigned short *__restrict__ kidx,
                                const bool fxForce
#ifdef SY_FX_LDS
                                , double *fxAcc
#endif
#ifdef SY_HDP_FUSED
                                , const int fxWindow
#endif
#endif
                                ) {
    const Geometry g = make_geometry(ring, ringD);
    const int lane = g.lane, wave = g.wave;
    const int lX = (int) it.lX, D = (int) (it.lX + it.lY);
    const double *cf = sh.coef;
#ifdef SY_VANILLA
    const double lYM = model[CP_VHDR_LOG_YM], lYY = model[CP_VHDR_LOG_YY];
    (void) lX;
#else
    const bool hasSwitchX = model[T_GAP_SWITCH_TO_X] > CP_NEG_INF;
    double T[9];
#pragma unroll
    for (int i = 0; i < 9; i++) T[i] = model[i];
#endif

    const int dTop = uni(ld_agent(&state->winTop)), tracedBackFrom = uni(ld_agent(&state->winFrom)),
              tracedBackTo = uni(ld_agent(&state->winTo));
    const bool atEnd = uni(ld_agent(&state->winAtEnd)) != 0;
    BPROF_DECL
    const int tPost0 = dTop < tracedBackFrom ? dTop : tracedBackFrom; /* first decoded diagonal */
    const int nPost = tPost0 - tracedBackTo;                         /* diagonals decoded      */
    band_stage(bf, bandTab, D, dTop - (SY_BAND_RING - 1), dTop);
    /* threshold 0: every in-band cell is a pair, one of exponent -inf too (exp(-inf) = 0 >= 0, :776-786), and the
     * candidates leave those out: the scan decodes the window, as in the wave kernels */
    if (threadIdx.x == 0) sh.scan = P.logThrSlack > CP_NEG_INF ? 0 : 1;
#ifdef SY_FUSED
    if (threadIdx.x == 0) SY_FX_REDO(sh) = fxForce ? 1 : 0;
#endif
    __syncthreads();
    /* Candidates for the posterior decode, collected by the sweep: a cell whose F.match + B.match
     * lies within SY_CAND_SLACK of the threshold, measured against an estimate of the window's
     * totalProbability taken at its first refresh.  Phase T checks every exact total of the window
     * against the estimate; if one strays (or a list overflows) the window is decoded by the scan. */
    const int candCap = SY_CAND_PER_DIAG * ringD;
    int2 *const myKx = candKx + (long long) wave * candCap;
    double *const myFb = candFb + (long long) wave * candCap;
    int nCand = 0;
    double candThr = CP_NEG_INF, totEst = CP_NEG_INF;

    /* ------------------------------ phase S: the sweep back ------------------------------ */
    /* (in the fused builds the sweep is a function that runs once or twice; exact: the second sweep of a window, its
     * terms taken against the exact totals phase T left) */
#ifdef SY_FUSED
    auto sweep = [&](const bool exact) __attribute__((always_inline)) {
        if (exact) { /* the band ring has moved down with the first sweep: back to the window's top */
            band_stage(bf, bandTab, D, dTop - (SY_BAND_RING - 1), dTop);
            __syncthreads();
        }
#else
    {
#endif
        int bxmin, bxmax;                 /* band of diagonal t   */
        band_get(bf, dTop, bxmin, bxmax);
        int nxmin = bxmin, nxmax = bxmax; /* band of diagonal t+1 */
        int pxmin, pxmax;                 /* band of diagonal t-1 */
        band_get(bf, dTop - 1, pxmin, pxmax);

        int xs = wave * 64 + lane;        /* backward representative: xmax-P < x <= xmax */
        xs += ((bxmin - xs + SY_P - 1) / SY_P) * SY_P;
        if (xs > bxmax) xs -= SY_P;
        bool tvalid = xs >= bxmin;        /* slot in band on diagonal t */
        double Bm, Bx, By;                                        /* backward cell on diagonal t        */
        /* What a cell hands to the diagonals below are sums B + (eP + tP) of its own backward value, its own
         * emission and a transition.  The slot above sends the two ingredients (B.match with its match emission,
         * B.gapX with its gap-X emission) down the lanes and the receiver forms the sums: four values to shift and
         * to hold instead of eight; the sums are the same expressions, so the doubles are the same. */
#ifdef SY_VANILLA
        /* Under the vanilla machine a step's transitions are those of the cell it goes TO, and the slot above owns
         * that cell's column: it sends the sums themselves, B + (eP + tP) per from-state, in the reference's grouping
         * -- three for the middle block, two for the lower block (no emission: B + (0 + tP) is B + tP).  The middle
         * block's sums are formed on the diagonal their cell is on, with the transitions the slot holds THEN: two
         * diagonals later, when they are used, the slot may have passed to another k-mer. */
        double hM0 = CP_NEG_INF, hM1 = CP_NEG_INF, hM2 = CP_NEG_INF; /* middle-block sums of slot+1 on t+2 */
        double S0 = 0.0, S1 = 0.0, S2 = 0.0; /* match emission of t+1 plus each transition into match, as of t+1 */
#else
        double hB = CP_NEG_INF, hP = 0.0;        /* B.match and match emission of slot+1 on t+2 (middle block) */
        double pmPrev = 0.0;                     /* match emission of t+1 */
#endif
        double Um = CP_NEG_INF, Uy = CP_NEG_INF; /* upper-block sums from t+1 (same slot)                       */
        double BmPrev = CP_NEG_INF;              /* backward match of t+1 */
        {
            double e0, e1, e2; /* end state vector (stateMachine.c:1179-1207) */
#ifdef SY_VANILLA
            /* stateMachine3Vanilla_endStateProb / _raggedEndStateProb (stateMachine.c:1209-1236) */
            const double endM = model[CP_VHDR_END_M], endX = model[CP_VHDR_END_X], endY = model[CP_VHDR_END_Y];
            e0 = atEnd && it.raggedR ? (endX + endY) / 2.0 : endM;
            e1 = endX;
            e2 = endY;
#else
            if (atEnd && it.raggedR) {
                e0 = (T[T_GAP_OPEN_X] + T[T_GAP_OPEN_Y]) / 2.0;
                e1 = T[T_GAP_EXTEND_X];
                e2 = T[T_GAP_EXTEND_Y];
            } else {
                e0 = T[T_MATCH_CONTINUE];
                e1 = T[T_MATCH_FROM_GAP_X];
                e2 = T[T_MATCH_FROM_GAP_Y];
            }
#endif
            Bm = tvalid ? e0 : CP_NEG_INF;
            Bx = tvalid ? e1 : CP_NEG_INF;
            By = tvalid ? e2 : CP_NEG_INF;
        }
        /* the sweep needs one constant per k-mer, its gap-X emission: held per slot, refreshed from
         * a 64-k-mer chunk when a k-mer enters at the low edge of the band */
#ifdef SY_VANILLA
        /* ... under the vanilla machine its five log transition probabilities, from the LDS ring (TransFeed) */
        double tr[5];
#pragma unroll
        for (int j = 0; j < 5; j++) tr[j] = track[(long long) (tvalid ? xs : 0) * SY_ROW + SY_TR + j];
        int xinB = bxmin - 1; /* k-mers above xinB are installed */
        int trLo = xinB - SY_TR_AHEAD > 0 ? xinB - SY_TR_AHEAD : 0; /* lowest k-mer staged */
        trans_stage(tf, track, trLo, xinB);
#else
        double pxReg = track[(long long) (tvalid ? xs : 0) * CP_ROW + CP_GAPX];
        int xinB = bxmin - 1; /* k-mers above xinB are installed */
        int pxBase = (xinB >= 0 ? xinB : 0) & ~63;
        double pxChunk = track[(long long) min(pxBase + lane, lX) * CP_ROW + CP_GAPX];
#endif

        /*
         * The forward match cell and the two emissions of a diagonal are fetched SY_PREFETCH diagonals
         * before the sweep reaches it: a wave that waits for a load also waits for everything issued
         * before it (vmcnt is one in-order queue), so a fetch consumed one diagonal later costs a full
         * HBM round trip per diagonal.  The loop is unrolled by the prefetch depth so that each
         * in-flight diagonal has registers of its own and the waits are exact counts.  The loads are
         * unconditional (no branch, so the counts hold): a lane whose slot cannot be in the band on
         * that diagonal reads a fixed dummy line instead, and every value is masked when consumed
         * (only cells of the band are ever stored to the ring; other slots hold stale data).
         */
        auto fetch = [&](const int tt, const bool want, double &f, double &pm, double &py SY_FXQ(double &fx, double &fy))
                         __attribute__((always_inline)) {
            const double *p = want ? g.rp(tt, 0) : g.rw;
            f = p[0];
            pm = p[3 * 64];
            py = p[4 * 64];
#ifdef SY_FUSED /* the fused E-step reads the row's two gap states too (the vanilla machine's: gap X) */
            fx = p[1 * 64];
#ifndef SY_VANILLA
            fy = p[2 * 64];
#endif
#endif
        };
        int calcs = 0, nTotWin = 0;
        int xsN = xs; /* this slot's k-mer on diagonal t+1 */
#if defined(SY_FUSED) && defined(SY_VANILLA)
        /*
         * The terms of diagonalCalculation_Expectations (:841-863 with cell_signal_updateBetaAndAlphaProb :478-498), those
         * cpecan_k_sy_expect (vanilla form) takes from the two rings: match -> gap X (beta) and gap X -> gap X (alpha), from
         * the cell's lower neighbour, into the skip bin of the cell's column.  A slot that holds the forward cell (t, x)
         * also holds, shifted down from the slot above, B.gapX of the cell (t+1, x+1) and that column's a_mx and a_xx --
         * what the backward recurrence's lower block gathers from.  Each term is taken against the total of diagonal t+1:
         * the window's estimate, or on the second sweep the exact total of that diagonal's segment.  Sums per segment:
         * beta and alpha of the column the slot points at (gCol = x + 1), in registers: five VGPRs, and keeping them in LDS
         * brings no occupancy step in reach (SY_BACKWARD_ATTR).
         */
        double beta = 0.0, alpha = 0.0, refX = exact ? uni_d(ld_agent(&wtot[0].total)) : 0.0;
        int gCol = -1, segAcc = 0;
        const int fxSlot = wave * 64 + lane;
        fxo.c[fxSlot] = -1; /* segment 0 has no A record yet */
        auto fx_flush = [&]() __attribute__((always_inline)) {
            fxo.g[((segAcc * 2 + 1) * SY_P + fxSlot) * 2 + 0] = beta;
            fxo.g[((segAcc * 2 + 1) * SY_P + fxSlot) * 2 + 1] = alpha;
            fxo.c[(segAcc * 2 + 1) * SY_P + fxSlot] = gCol;
            fxo.c[(segAcc * 2 + 2) * SY_P + fxSlot] = -1; /* the next segment's A record */
            beta = alpha = 0.0;
            segAcc++;
            if (exact) refX = uni_d(ld_agent(&wtot[segAcc].total));
        };
        /* fM, fX: the slot's forward cell on diagonal t (-inf outside the band), x its column, in: it is in the band; lB,
         * aMX, aXX: B.gapX of (t+1, x+1) and that column's two transitions; nMin..nMax the band of t+1.  Called with
         * t+1 <= tPost0. */
        auto fx_terms = [&](const int t, const bool on, const int x, const bool in, const double fM, const double fX,
                            const double lB, const double aMX, const double aXX, const int nMin, const int nMax)
                            __attribute__((always_inline)) {
            if (t + 2 <= tPost0 && (tPost0 - (t + 2)) % 10 == 9) fx_flush(); /* t+2 ended its segment */
            if (on) {
                const double ref = exact ? refX : totEst;
                /* (second sweep only) a total of -inf or NaN: every term is NaN, as in the reference, and the terms must
                 * then be those the reference forms -- a cell of the band whose lower neighbour is in the band too --
                 * instead of one per slot */
                const bool nf = exact && !(ref > CP_NEG_INF);
                /* exp() of anything below SY_FX_ZERO is +0: a wave none of whose lanes holds a larger exponent (or a NaN)
                 * -- most waves of a wide band, whose cells far from the alignment lie thousands of nats under the
                 * total -- adds its zeros without the two exp() calls, a third of the step's instructions */
                const double a0 = fM + lB + (0 + aMX) - ref, a1 = fX + lB + (0 + aXX) - ref;
                double p0 = 0.0, p1 = 0.0;
                if (__ballot(!(a0 < SY_FX_ZERO) || !(a1 < SY_FX_ZERO)) != 0ull) {
                    p0 = exp(a0);
                    p1 = exp(a1);
                }
                const bool inL = in && x + 1 >= nMin && x + 1 <= nMax; /* the cell (t+1, x+1) exists */
                if (nf) {
                    p0 = inL ? p0 : 0.0;
                    p1 = inL ? p1 : 0.0;
                }
                if (inL && x + 1 != gCol) { /* the slot points at another column than before */
                    if (beta != 0.0 || alpha != 0.0) {
                        fxo.g[((segAcc * 2) * SY_P + fxSlot) * 2 + 0] = beta;
                        fxo.g[((segAcc * 2) * SY_P + fxSlot) * 2 + 1] = alpha;
                        fxo.c[(segAcc * 2) * SY_P + fxSlot] = gCol;
                    }
                    beta = alpha = 0.0;
                    gCol = x + 1;
                }
                beta += p0;
                alpha += p1;
            }
        };
#elif defined(SY_FUSED)
        /*
         * The terms of diagonalCalculation_Expectations (:841-863 with cell_signal_updateTransAndKmerSkipExpectations
         * :426-443), those cpecan_k_sy_expect forms from the two rings.  A slot that holds the forward cell (t, x) also
         * holds, shifted down from the slot above or kept from the diagonal above, the backward half of every term that
         * starts at that cell: of the cell (t+2, x+1) B.match and the match emission (middle block: hB, hP), of (t+1, x+1)
         * B.gapX and the gap-X emission (lower block: rBx, rPx), of (t+1, x) the sums B.gapY + (gap-Y emission +
         * transition) (upper block: Um, Uy) -- what the backward recurrence gathers from.  Each term is taken against the
         * total of the diagonal of the cell it goes TO: the window's estimate, or on the second sweep the exact total of
         * that diagonal's segment.  Sums per segment: eight per lane (ea), and the gap-X terms of the column the slot
         * points at once more for that column's k-mer bin (gSum of column gCol = x + 1).
         */
        /* M>X X>X Y>X | M>M X>M Y>M | M>Y Y>Y */
#ifdef SY_FX_LDS
        double *const ea = fxAcc + threadIdx.x; /* (a thread reads and writes its own eight entries only: no barrier) */
#define SY_EA(i) ea[(i) * SY_P]
#else
        double ea[8];
#define SY_EA(i) ea[i]
#endif
#pragma unroll
        for (int i = 0; i < 8; i++) SY_EA(i) = 0.0;
        double refX = exact ? uni_d(ld_agent(&wtot[0].total)) : 0.0;
        int segAcc = 0;
#ifndef SY_HDP /* (the HDP machine collects no gap-X sums per k-mer: no g, no c) */
        double gSum = 0.0;
        int gCol = -1;
        const int fxSlot = wave * 64 + lane;
        fxo.c[fxSlot] = -1; /* segment 0 has no A record yet */
#endif
        auto fx_flush = [&]() __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < 8; i++) {
                double v = SY_EA(i);
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
                if (lane == 0) fxo.tr[(segAcc * SY_R + wave) * 8 + i] = v;
                SY_EA(i) = 0.0;
            }
#ifndef SY_HDP
            fxo.g[(segAcc * 2 + 1) * SY_P + fxSlot] = gSum;
            fxo.c[(segAcc * 2 + 1) * SY_P + fxSlot] = gCol;
            fxo.c[(segAcc * 2 + 2) * SY_P + fxSlot] = -1; /* the next segment's A record */
            gSum = 0.0;
#endif
            segAcc++;
            if (exact) refX = uni_d(ld_agent(&wtot[segAcc].total));
        };
        /* fM, fX, fY: the slot's forward cell on diagonal t (-inf outside the band), x its column, in: it is in the band;
         * nMin..nMax the band of t+1.  Called with t+1 <= tPost0, before this diagonal's backward cell replaces what the
         * slot holds of the two above. */
        auto fx_terms = [&](const int t, const bool on, const int x, const bool in, const double fM, const double fX,
                            const double fY, const double mB, const double mP, const double lB, const double lP,
                            const double uM, const double uY, const int nMin, const int nMax)
                            __attribute__((always_inline)) {
            /* (second sweep only) a total of -inf or NaN: every term is NaN, as in the reference, and the terms must then
             * be those the reference forms -- a cell of the band whose neighbour is in the band too, the gap Y -> gap X
             * term included where the model has none (its transition is -inf) -- instead of one per slot */
            if (t + 2 <= tPost0) { /* middle block of t+2 (skipped at the window's lowest diagonal: no forward[t-2]) */
                const double ref = exact ? refX : totEst;
                const bool nf = exact && !(ref > CP_NEG_INF);
                if (on) {
#ifdef SY_HDP_FUSED
                    /* The HDP machine's assignments (cell_signal_updateTransAndKmerSkipExpectations2 :445-476): a transition
                     * into match whose own posterior exp(s - total) reaches the threshold leaves as (from-state + 4 *
                     * window, x - 1, y - 1) of the cell it goes TO, (t+2, x+1), with its exponent.  s: the three exponents
                     * before the total is subtracted.  The first sweep parks (diagonal, from-state, column) and s where s
                     * lies within SY_CAND_SLACK of the threshold against the estimate -- a cell or a neighbour outside the
                     * band has s = -inf -- and the selection after phase T, which has the exact totals, takes s - total: the
                     * last operation of the ring path's expression, so its exponents bit for bit.  The second sweep has
                     * the totals and the band of t+2: it emits here, for the cells the reference visits, as
                     * cpecan_k_sy_expect does. */
                    const double s3 = fM + mB + (mP + T[T_MATCH_CONTINUE]), s4 = fX + mB + (mP + T[T_MATCH_FROM_GAP_X]),
                                 s5 = fY + mB + (mP + T[T_MATCH_FROM_GAP_Y]);
                    const double e3 = s3 - ref, e4 = s4 - ref, e5 = s5 - ref;
                    /* (skipping the three calls for a wave whose every exponent is below SY_FX_ZERO, as the vanilla fused
                     * sweep does, was measured and costs more than it saves: this machine's posteriors are flat) */
                    double p3 = exp(e3), p4 = exp(e4), p5 = exp(e5);
                    if (exact) {
                        int cMin, cMax;
                        band_load(bandTab, t + 2, cMin, cMax);
                        const bool ok = in && x + 1 >= cMin && x + 1 <= cMax;
                        const double ee[3] = { e3, e4, e5 }, qq[3] = { p3, p4, p5 };
#pragma unroll
                        for (int f = 0; f < 3; f++)
                            if (ok && qq[f] >= P.threshold) {
                                const long long at = (long long) atomicAdd((unsigned long long *) &state->nPairs, 1ull);
                                if (at < out.pairCap) {
                                    long long *o = out.pairs + at * 3;
                                    o[0] = f + 4ll * fxWindow;
                                    o[1] = x;     /* (x + 1) - 1 */
                                    o[2] = t - x; /* ((t + 2) - (x + 1)) - 1 */
                                    out.logp[at] = ee[f];
                                }
                            }
                        if (nf) {
                            p3 = ok ? p3 : 0.0;
                            p4 = ok ? p4 : 0.0;
                            p5 = ok ? p5 : 0.0;
                        }
                    } else {
                        const double ss[3] = { s3, s4, s5 };
#pragma unroll
                        for (int f = 0; f < 3; f++) {
                            const bool hit = ss[f] >= candThr;
                            const unsigned long long hm = __ballot(hit);
                            if (hm != 0ull) {
                                const int ci = nCand + __popcll(hm & ((1ull << lane) - 1ull));
                                if (hit && ci < candCap) { /* (writes stop at the capacity, the count goes on) */
                                    myKx[ci] = make_int2((tPost0 - (t + 2)) * 4 + f, x + 1);
                                    myFb[ci] = ss[f];
                                }
                                nCand += __popcll(hm);
                            }
                        }
                    }
#else
                    double p3 = exp(fM + mB + (mP + T[T_MATCH_CONTINUE]) - ref);
                    double p4 = exp(fX + mB + (mP + T[T_MATCH_FROM_GAP_X]) - ref);
                    double p5 = exp(fY + mB + (mP + T[T_MATCH_FROM_GAP_Y]) - ref);
                    if (nf) {
                        int cMin, cMax;
                        band_load(bandTab, t + 2, cMin, cMax);
                        const bool ok = in && x + 1 >= cMin && x + 1 <= cMax;
                        p3 = ok ? p3 : 0.0;
                        p4 = ok ? p4 : 0.0;
                        p5 = ok ? p5 : 0.0;
                    }
#endif
                    SY_EA(3) += p3;
                    SY_EA(4) += p4;
                    SY_EA(5) += p5;
                }
                if ((tPost0 - (t + 2)) % 10 == 9) fx_flush(); /* t+2 ends its segment */
            }
            if (on) { /* lower and upper blocks of t+1 */
                const double ref = exact ? refX : totEst;
                const bool nf = exact && !(ref > CP_NEG_INF);
                double p0 = exp(fM + lB + (lP + T[T_GAP_OPEN_X]) - ref);
                double p1 = exp(fX + lB + (lP + T[T_GAP_EXTEND_X]) - ref);
                double p2 = hasSwitchX ? exp(fY + lB + (lP + T[T_GAP_SWITCH_TO_X]) - ref) : 0.0;
                double p6 = exp(fM + uM - ref);
                double p7 = exp(fY + uY - ref);
                const bool inL = in && x + 1 >= nMin && x + 1 <= nMax; /* the cell (t+1, x+1) exists */
                if (nf) {
                    const bool inU = in && x >= nMin && x <= nMax;     /* the cell (t+1, x) */
                    p0 = inL ? p0 : 0.0;
                    p1 = inL ? p1 : 0.0;
                    p2 = inL ? (hasSwitchX ? p2 : exp(CP_NEG_INF - ref)) : 0.0;
                    p6 = inU ? p6 : 0.0;
                    p7 = inU ? p7 : 0.0;
                }
                SY_EA(0) += p0;
                SY_EA(1) += p1;
                if (hasSwitchX || nf) SY_EA(2) += p2;
#ifndef SY_HDP
                if (inL && x + 1 != gCol) { /* the slot points at another column than before */
                    if (gSum != 0.0) {
                        fxo.g[(segAcc * 2) * SY_P + fxSlot] = gSum;
                        fxo.c[(segAcc * 2) * SY_P + fxSlot] = gCol;
                    }
                    gSum = 0.0;
                    gCol = x + 1;
                }
                gSum += p0;
                gSum += p1;
                if (hasSwitchX || nf) gSum += p2;
#endif
                SY_EA(6) += p6;
                SY_EA(7) += p7;
            }
        };
#undef SY_EA
#endif
        auto step = [&](const int t, double &qF, double &qPm, double &qPy SY_FXQ(double &qFx, double &qFy))
                        __attribute__((always_inline)) {
            const bool active = row_active(wave, bxmin, bxmax);
            const bool activeN = row_active(wave, nxmin, nxmax);
            if (t < dTop) {
                xsN = xs;
                if (xs > bxmax) xs -= SY_P;
            }
            const bool vt = xs >= bxmin;
            const double fMc = vt ? qF : CP_NEG_INF, pmc = vt ? qPm : 0.0, pyc = vt ? qPy : 0.0;
#if defined(SY_FUSED) && defined(SY_VANILLA)
            const double fXc = vt ? qFx : CP_NEG_INF;
#elif defined(SY_FUSED)
            const double fXc = vt ? qFx : CP_NEG_INF, fYc = vt ? qFy : CP_NEG_INF;
#endif
            /* the slot's k-mer SY_PREFETCH diagonals down is xs or out of band (bands <= SY_P - 2 * depth) */
            fetch(t - SY_PREFETCH, xs >= bxmin - SY_PREFETCH, qF, qPm, qPy SY_FXQ(qFx, qFy));
            if (t < dTop) {
                lds_barrier();
                const double *xa = sh.xch[(t + 1) & 1][g.waveAbove];
#ifdef SY_VANILLA
                /* of slot+1 on t+1: the lower block's sums (used now) and the middle block's (one diagonal further
                 * down); tr[] is still that diagonal's here */
#ifdef SY_FUSED
                /* (the fused terms take B.gapX and the two transitions apart, so those travel and the lower block's
                 * sums are formed here: the same operands, the same doubles) */
                const double rBx = shl1(xa[5], Bx), rA0 = shl1(xa[6], tr[0]), rA1 = shl1(xa[7], tr[1]);
                const double rX0 = rBx + rA0, rX1 = rBx + rA1;
#else
                const double rX0 = shl1(xa[0], Bx + tr[0]), rX1 = shl1(xa[1], Bx + tr[1]);
#endif
                const double rM0 = shl1(xa[2], Bm + S0), rM1 = shl1(xa[3], Bm + S1), rM2 = shl1(xa[4], Bm + S2);
                const bool bvalid = xs >= bxmin;
                while (xinB >= bxmin) {
                    if (SY_WAVE_OF(xinB) == wave && lane == (xinB & 63)) {
                        const double *r = tf.r + (xinB & (SY_TR_RING - 1)) * 5;
#pragma unroll
                        for (int j = 0; j < 5; j++) tr[j] = r[j];
                    }
                    xinB--;
                }
#else
                /* of slot+1 on t+1: B.gapX with its k-mer's gap-X emission (lower block of t+1), B.match with its
                 * match emission (middle block, used one diagonal further down) */
                const double rBx = shl1(xa[0], Bx), rPx = shl1(xa[1], pxReg);
                const double rBm = shl1(xa[2], Bm), rPm = shl1(xa[3], pmPrev);
                const bool bvalid = xs >= bxmin;
                while (xinB >= bxmin) {
                    if (xinB < pxBase) {
                        pxBase -= 64;
                        pxChunk = track[(long long) min(pxBase + lane, lX) * CP_ROW + CP_GAPX];
                    }
                    const double v = bcast(pxChunk, xinB - pxBase);
                    if (SY_WAVE_OF(xinB) == wave) pxReg = set_lane(pxReg, xinB & 63, v);
                    xinB--;
                }
#endif
#if defined(SY_FUSED) && defined(SY_VANILLA)
                if (t + 1 <= tPost0) fx_terms(t, active, xs, bvalid, fMc, fXc, rBx, rA0, rA1, nxmin, nxmax);
#elif defined(SY_FUSED)
                if (t + 1 <= tPost0)
                    fx_terms(t, active, xs, bvalid, fMc, fXc, fYc, hB, hP, rBx, rPx, Um, Uy, nxmin, nxmax);
#endif
                BmPrev = Bm;
                tvalid = bvalid;
                double bm = CP_NEG_INF, bx = CP_NEG_INF, by = CP_NEG_INF;
                if (active) {
                    /* gather form of cell_calculateBackward: (t+2) middle block, then (t+1, smaller
                     * x-y) upper block, then (t+1, larger x-y) lower block */
#ifdef SY_VANILLA
                    bm = ladd(ladd(hM0, Um, cf), rX0, cf);
                    bx = ladd(hM1, rX1, cf);
                    by = ladd(hM2, Uy, cf);
#else
                    bm = ladd(ladd(hB + (hP + T[T_MATCH_CONTINUE]), Um, cf), rBx + (rPx + T[T_GAP_OPEN_X]), cf);
                    bx = ladd(hB + (hP + T[T_MATCH_FROM_GAP_X]), rBx + (rPx + T[T_GAP_EXTEND_X]), cf);
                    by = ladd(hB + (hP + T[T_MATCH_FROM_GAP_Y]), Uy, cf);
                    if (hasSwitchX) by = ladd(by, rBx + (rPx + T[T_GAP_SWITCH_TO_X]), cf);
#endif
                    bm = bvalid ? bm : CP_NEG_INF;
                    bx = bvalid ? bx : CP_NEG_INF;
                    by = bvalid ? by : CP_NEG_INF;
                }
                Bm = bm; Bx = bx; By = by;
#ifdef SY_VANILLA
                hM0 = rM0; hM1 = rM1; hM2 = rM2;
#else
                hB = rBm; hP = rPm;
#endif
            }
            /* what this diagonal hands down: the upper-block sums stay in the slot (a cell outside the band has
             * B = -inf and a zero emission: the sums are -inf by themselves); the rest leaves as B and emission */
#ifdef SY_VANILLA
            Um = By + (pyc + tr[4]);
            Uy = By + (pyc + lYY);
            const double nS0 = pmc + tr[2], nS1 = pmc + tr[3], nS2 = pmc + lYM;
            if (lane == 0) {
                double *x = sh.xch[t & 1][wave];
#ifdef SY_FUSED
                x[5] = Bx; x[6] = tr[0]; x[7] = tr[1]; x[2] = Bm + nS0; x[3] = Bm + nS1; x[4] = Bm + nS2;
#else
                x[0] = Bx + tr[0]; x[1] = Bx + tr[1]; x[2] = Bm + nS0; x[3] = Bm + nS1; x[4] = Bm + nS2;
#endif
            }
#else
            Um = By + (pyc + T[T_GAP_OPEN_Y]);
            Uy = By + (pyc + T[T_GAP_EXTEND_Y]);
            if (lane == 0) {
                double *x = sh.xch[t & 1][wave];
                x[0] = Bx; x[1] = pxReg; x[2] = Bm; x[3] = pmc;
            }
#endif

            if (t <= tracedBackFrom) {
                const double fb = fMc + Bm;
#ifdef SY_FUSED
                if (calcs++ % 10 == 0 && !exact) { /* (the second sweep of a window has its totals) */
#else
                if (calcs++ % 10 == 0) {
#endif
                    /* per-cell terms of diagonalCalculationTotalProbability (:736-754), folded in
                     * phase T: v = cell_dotProduct(forward[t], backward[t]) (:391-397) ... */
                    const bool second = t + 1 <= dTop;
                    double v = CP_NEG_INF, w = CP_NEG_INF;
                    /* all five loads of a refresh go out together (one HBM round trip, not two: the store of
                     * v below would otherwise fence the second group behind the first); masked when used */
                    const bool below = second && activeN && xsN - 1 >= pxmin && xsN - 1 <= pxmax;
#ifdef SY_ABLATE_TOTLOADS
                    const double fx = fMc, fy = fMc, r0 = fMc, r1 = fMc, r2 = fMc;
#else
                    const double *pa = tvalid ? g.rp(t, 1) : g.rw, *pb = below ? g.rpb(t - 1, 0) : g.rw;
                    const double fx = pa[0], fy = pa[64], r0 = pb[0], r1 = pb[64], r2 = pb[128];
#endif
                    if (tvalid) {
                        v = fb;
                        v = ladd(v, fx + Bx, cf);
                        v = ladd(v, fy + By, cf);
                        vw[((long long) nTotWin * 2 + 0) * SY_P + wave * 64 + lane] = v;
                    }
                    if (second && activeN) {
                        /* ... and w = matches stepping over t: forward[t-1] --match--> the cells of
                         * t+1, dotted with backward[t+1] (only the match state of that clone is
                         * ever above -inf) */
                        const double s0 = below ? r0 : CP_NEG_INF, s1 = below ? r1 : CP_NEG_INF,
                                     s2 = below ? r2 : CP_NEG_INF;
#ifdef SY_VANILLA
                        /* (the transitions of the cell on t+1, which this slot held then: S0..S2) */
                        double mm = s0 + S0;
                        mm = ladd(mm, s1 + S1, cf);
                        mm = ladd(mm, s2 + S2, cf);
#else
                        double mm = s0 + (pmPrev + T[T_MATCH_CONTINUE]);
                        mm = ladd(mm, s1 + (pmPrev + T[T_MATCH_FROM_GAP_X]), cf);
                        mm = ladd(mm, s2 + (pmPrev + T[T_MATCH_FROM_GAP_Y]), cf);
#endif
                        w = mm + BmPrev;
                        vw[((long long) nTotWin * 2 + 1) * SY_P + wave * 64 + lane] = w;
                    }
                    if (nTotWin == 0) {
                        /* the estimate: the same terms folded in any order (it only steers the
                         * candidate test; the exact, ordered folds are phase T's) */
                        double acc = wave_fold(CP_NEG_INF, v, cf);
                        acc = wave_fold(acc, w, cf);
                        if (lane == 0) sh.vbuf[wave] = acc;
                        lds_barrier();
                        double est = sh.vbuf[0];
#pragma unroll
                        for (int q = 1; q < SY_R; q++) est = ladd(est, sh.vbuf[q], cf);
                        totEst = est;
                        candThr = est + (P.logThrSlack - SY_CAND_SLACK);
                    }
                    if (threadIdx.x == 0) {
                        WinTotal w;
                        w.t = t; w.xmin = bxmin; w.xmax = bxmax; w.nxmin = nxmin; w.nxmax = nxmax;
                        w.second = second ? 1 : 0;
                        w.total = CP_NEG_INF;
                        wtot[nTotWin] = w;
                    }
                    nTotWin++;
                }
                /* exponent of the posterior, less the total: parked in the emission slot this diagonal
                 * no longer needs (the forward cells themselves stay intact: the next window's
                 * refresh at its lowest diagonal reads forward[tracedBackFrom], :944,:985) */
                if (SY_MODE(P) != 0) {
                    /* Baum-Welch: the backward cell goes to its own ring for the expectation kernel
                     * (the emissions in slots 3, 4 stay: that kernel re-uses them); the fused E-step has used it */
                    if (tvalid && !SY_FX) {
                        double *b = bring + (long long) (t & g.ringMask) * (SY_R * SY_BRING_VALUES * 64)
                                    + wave * (SY_BRING_VALUES * 64) + lane;
#ifdef SY_VANILLA
                        b[0] = Bx; /* (all that machine's expectation kernel reads of the cell) */
#else
                        b[0] = Bm;
                        b[64] = Bx;
                        b[128] = By;
#endif
                    }
                }
#ifndef SY_ABLATE_FB
                else if (tvalid) *g.rp(t, 3) = fb;
#endif
                const bool cand = SY_MODE(P) == 0 && tvalid && fb >= candThr && fb > CP_NEG_INF;
                const unsigned long long cm = __ballot(cand);
                if (cm != 0ull) {
                    const int ci = nCand + __popcll(cm & ((1ull << lane) - 1ull));
                    if (cand && ci < candCap) {
                        myKx[ci] = make_int2(tPost0 - t, xs);
                        myFb[ci] = fb;
                    }
                    nCand += __popcll(cm);
                }
            }
#ifdef SY_VANILLA
            S0 = nS0; S1 = nS1; S2 = nS2;
#else
            pmPrev = pmc;
#endif
            nxmin = bxmin; nxmax = bxmax;
            bxmin = pxmin; bxmax = pxmax;
            if (t - 2 >= tracedBackTo) band_get(bf, t - 2, pxmin, pxmax);
        };
        double q0F, q0Pm, q0Py, q1F, q1Pm, q1Py, q2F, q2Pm, q2Py, q3F, q3Pm, q3Py;
#if defined(SY_FUSED) && defined(SY_VANILLA)
        double q0Fx, q1Fx, q2Fx, q3Fx;
#elif defined(SY_FUSED)
        double q0Fx, q0Fy, q1Fx, q1Fy, q2Fx, q2Fy, q3Fx, q3Fy;
#endif
        {
            const bool want = xs >= bxmin - SY_PREFETCH;
            fetch(dTop, want, q0F, q0Pm, q0Py SY_FXQ(q0Fx, q0Fy));
            fetch(dTop - 1, want, q1F, q1Pm, q1Py SY_FXQ(q1Fx, q1Fy));
            fetch(dTop - 2, want, q2F, q2Pm, q2Py SY_FXQ(q2Fx, q2Fy));
            fetch(dTop - 3, want, q3F, q3Pm, q3Py SY_FXQ(q3Fx, q3Fy));
        }
        int t = dTop, bandLo = dTop - (SY_BAND_RING - 1); /* lowest diagonal whose band is staged */
#pragma unroll 1
        for (; t - (SY_PREFETCH - 1) > tracedBackTo; t -= SY_PREFETCH) {
            if (t - 64 < bandLo) { /* 32 more band entries, long before the sweep reads them */
                band_stage(bf, bandTab, D, bandLo - 32, bandLo - 1);
                bandLo -= 32;
#ifdef SY_VANILLA
                /* ... and the transitions of the k-mers that can enter before the next refill */
                const int lo = xinB - SY_TR_AHEAD > 0 ? xinB - SY_TR_AHEAD : 0;
                if (lo < trLo) {
                    trans_stage(tf, track, lo, trLo - 1);
                    trLo = lo;
                }
#endif
            }
            step(t, q0F, q0Pm, q0Py SY_FXQ(q0Fx, q0Fy));
            step(t - 1, q1F, q1Pm, q1Py SY_FXQ(q1Fx, q1Fy));
            step(t - 2, q2F, q2Pm, q2Py SY_FXQ(q2Fx, q2Fy));
            step(t - 3, q3F, q3Pm, q3Py SY_FXQ(q3Fx, q3Fy));
        }
        /* the last diagonals of the window (fewer than the prefetch depth): fetched on the spot */
#pragma unroll 1
        for (; t > tracedBackTo; t--) {
            double f, pm, py SY_FXQ(fx, fy);
            fetch(t, true, f, pm, py SY_FXQ(fx, fy));
            step(t, f, pm, py SY_FXQ(fx, fy));
        }
#ifdef SY_FUSED
        if (tPost0 > tracedBackTo) {
            /* the terms that start at the forward cells of tracedBackTo, the diagonal below the window: lower and upper
             * block of the window's lowest diagonal, middle block of the one above it (the bands have moved on: bxmin ..
             * bxmax is that diagonal's, nxmin .. nxmax the lowest decoded one's) */
            if (xs > bxmax) xs -= SY_P;
            const bool vt = xs >= bxmin;
#ifdef SY_VANILLA
            double f, pm, py, fx;
            fetch(tracedBackTo, vt, f, pm, py, fx);
            lds_barrier();
            const double *xa = sh.xch[(tracedBackTo + 1) & 1][g.waveAbove];
            const double rBx = shl1(xa[5], Bx), rA0 = shl1(xa[6], tr[0]), rA1 = shl1(xa[7], tr[1]);
            fx_terms(tracedBackTo, row_active(wave, bxmin, bxmax), xs, vt, vt ? f : CP_NEG_INF, vt ? fx : CP_NEG_INF,
                     rBx, rA0, rA1, nxmin, nxmax);
#else
            double f, pm, py, fx, fy;
            fetch(tracedBackTo, vt, f, pm, py, fx, fy);
            lds_barrier();
            const double *xa = sh.xch[(tracedBackTo + 1) & 1][g.waveAbove];
            const double rBx = shl1(xa[0], Bx), rPx = shl1(xa[1], pxReg);
            fx_terms(tracedBackTo, row_active(wave, bxmin, bxmax), xs, vt, vt ? f : CP_NEG_INF, vt ? fx : CP_NEG_INF,
                     vt ? fy : CP_NEG_INF, hB, hP, rBx, rPx, Um, Uy, nxmin, nxmax);
#endif
            fx_flush();
        }
#endif
#ifdef SY_FUSED
        if (!exact) sh.item = nTotWin;
    };
    sweep(false);
#ifdef SY_HDP_FUSED
    /* a wave's count of parked assignments, for the selection; a list that overflowed sends the window down the
     * second sweep */
    if (lane == 0) sh.cnt[1][wave][0] = nCand;
    if (nCand > candCap) SY_FX_REDO(sh) = 1;
#endif
#else
        sh.item = nTotWin;
        if (lane == 0) sh.cnt[1][wave][0] = nCand;
        if (nCand > candCap) sh.scan = 1;
    }
#endif
    __syncthreads(); /* the ring rows written above are read by other waves below */
    const int nTotWin = sh.item;

    BPROF(1)
    /* ------------------------------ phase T: the totals ------------------------------ */
#pragma unroll 1
    for (int k = threadIdx.x; k < 2 * nTotWin; k += SY_P) {
        const WinTotal w = wtot[k >> 1];
        const int f = k & 1;
        double acc = CP_NEG_INF;
        if (f == 0 || w.second) {
            const int lo = f ? w.nxmin : w.xmin, hi = f ? w.nxmax : w.xmax;
            const double *src = vw + ((long long) (k >> 1) * 2 + f) * SY_P;
            double v[8], nv[8]; /* the next eight terms are in flight while these eight are folded */
#pragma unroll
            for (int j = 0; j < 8; j++) v[j] = lo + j <= hi ? src[SY_SLOT(lo + j)] : CP_NEG_INF;
#pragma unroll 1
            for (int x0 = lo; x0 <= hi; x0 += 8) {
#pragma unroll
                for (int j = 0; j < 8; j++)
                    nv[j] = x0 + 8 + j <= hi ? src[SY_SLOT(x0 + 8 + j)] : CP_NEG_INF;
#pragma unroll
                for (int j = 0; j < 8; j++) acc = ladd(acc, v[j], cf); /* dpDiagonal_dotProduct :587-597 */
#pragma unroll
                for (int j = 0; j < 8; j++) v[j] = nv[j];
            }
        }
        sh.vbuf[threadIdx.x] = acc;
        __builtin_amdgcn_wave_barrier();
        if (f == 0) {
            double tot = acc;
            if (w.second) tot = ladd(acc, sh.vbuf[threadIdx.x + 1], cf);
            wtot[k >> 1].total = tot;
            if (!(fabs(tot - totEst) <= SY_CAND_SLACK)) sh.scan = 1; /* also catches NaN and infinities */
#ifdef SY_HDP_FUSED
            /* (the parked assignments are complete only where every total lies within SY_CAND_SLACK of the estimate: one
             * redo rule for sums and assignments) */
            if (!(fabs(tot - totEst) <= SY_CAND_SLACK)) SY_FX_REDO(sh) = 1;
#elif defined(SY_FUSED)
            if (!(fabs(tot - totEst) <= SY_FX_EST_BOUND)) SY_FX_REDO(sh) = 1;
#endif
            const long long o = out.nTot + (k >> 1);
            if (o < out.totCap) {
                out.totXay[o] = w.t;
                out.totVal[o] = tot;
            }
        }
    }
    out.nTot += nTotWin;
    __syncthreads();
#ifdef SY_FUSED
    /* the window's sums into the model's: scaled from the estimate, or taken once more against the exact totals where
     * the estimate is not finite or lies more than SY_FX_EST_BOUND from one of them (or the caller forces it) */
    if (nPost > 0) {
#ifdef SY_HDP_FUSED
        const bool redo = SY_FX_REDO(sh) != 0 || sh.scan != 0; /* (scan: a threshold without a logarithm, a total astray) */
#else
        const bool redo = SY_FX_REDO(sh) != 0;
#endif
        if (redo) {
            sweep(true);
            __syncthreads();
        }
#ifdef SY_VANILLA
        fx_finish(it, fxo, wtot, nTotWin, tPost0, tracedBackTo, totEst, redo, expect, track, sh.wbuf);
        (void) kidx;
#else
        fx_finish(it, fxo, wtot, nTotWin, tPost0, tracedBackTo, totEst, redo, expect, kidx);
#endif
#ifdef SY_HDP_FUSED
        /* the selection: every wave walks its own list of parked assignments; one leaves where exp(s - total) reaches the
         * threshold, the test and the record of cpecan_k_sy_expect (HDP form), in whatever order the lanes get there (the
         * host restores the reference's at fetch).  A window that went down the second sweep has emitted there. */
        if (!redo) {
            const int nC = sh.cnt[1][wave][0];
#pragma unroll 1
            for (int i = lane; i < nC; i += 64) {
                const int2 kx = myKx[i];
                const int k = kx.x >> 2, f = kx.x & 3, x = kx.y, t = tPost0 - k;
                const double e = myFb[i] - wtot[k / 10].total;
                if (exp(e) >= P.threshold) {
                    const long long at = (long long) atomicAdd((unsigned long long *) &state->nPairs, 1ull);
                    if (at < out.pairCap) {
                        long long *o = out.pairs + at * 3;
                        o[0] = f + 4ll * fxWindow;
                        o[1] = x - 1;
                        o[2] = (t - x) - 1;
                        out.logp[at] = e;
                    }
                }
            }
        }
#endif
    }
#endif

    BPROF(2)
    /* ------------------------------ phase D: the aligned pairs ------------------------------ */
    /*
     * Two passes over the window's diagonals; in both, every wave walks ALL diagonals but looks only
     * at its own 64 slots (the sweep's mapping), SY_DECODE_U diagonals per iteration with their loads
     * issued together, so HBM latency is paid once per batch instead of once per diagonal.
     *   pass 0  marks the hits: one 64-bit lane mask per (diagonal, wave) to scratch;
     *   prefix  hits per diagonal -> exclusive offsets in emission order (diagonals descending);
     *   pass 1  re-reads only the hit lanes, ranks each hit inside its diagonal by k-mer index
     *           (the reference's x-y order) from the diagonal's masks, and writes the triples.
     */
    if (SY_MODE(P) == 0 && nPost > 0) {
        int *const off = cntBuf;
        auto lane64 = [&](const unsigned long long v, const int src) __attribute__((always_inline)) {
            const unsigned lo = (unsigned) __builtin_amdgcn_readlane((int) (unsigned) v, src);
            const unsigned hi = (unsigned) __builtin_amdgcn_readlane((int) (unsigned) (v >> 32), src);
            return ((unsigned long long) hi << 32) | lo;
        };
        /* masks are written by one wave (or by atomics) and read by the others: read them at agent
         * scope so that a line cached by this CU earlier cannot be served stale */
        auto ld_msk = [&](const long long i) __attribute__((always_inline)) {
            return __hip_atomic_load(msk + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        };
        auto hits_of = [&](const int k) __attribute__((always_inline)) {
            int n = 0; /* masks are kept SY_MSK to a diagonal */
#pragma unroll
            for (int w2 = 0; w2 < SY_R; w2++) n += __popcll(ld_msk(k * (long long) SY_MSK + w2));
            return n;
        };
        auto prefix = [&]() __attribute__((always_inline)) {
                /* hits per diagonal from the masks; exclusive prefix in emission order */
                int *part = (int *) sh.wbuf;
                int carry = 0; /* hits of the rounds before this one */
#pragma unroll 1
                for (int base = 0; base < nPost; base += 8 * SY_P) { /* eight diagonals per thread and round */
                    const int b0 = base + (int) threadIdx.x * 8;
                    int h[8];
                    int sum = 0;
#pragma unroll
                    for (int j = 0; j < 8; j++) {
                        h[j] = b0 + j < nPost ? hits_of(b0 + j) : 0;
                        sum += h[j];
                    }
                    /* exclusive scan over the workgroup's threads: shuffles inside a wave, LDS across the waves */
                    int inc = sum;
#pragma unroll
                    for (int o2 = 1; o2 < 64; o2 <<= 1) {
                        const int up = __shfl_up(inc, o2);
                        if (lane >= o2) inc += up;
                    }
                    __syncthreads(); /* part[] of the previous round has been read */
                    if (lane == 63) part[wave] = inc;
                    __syncthreads();
                    int o = carry + inc - sum;
#pragma unroll
                    for (int w2 = 0; w2 < SY_R; w2++) {
                        const int c = part[w2];
                        if (w2 < wave) o += c;
                    }
#pragma unroll
                    for (int w2 = 0; w2 < SY_R; w2++) carry += part[w2];
#pragma unroll
                    for (int j = 0; j < 8; j++)
                        if (b0 + j < nPost) {
                            off[b0 + j] = o;
                            o += h[j];
                        }
                }
                if (threadIdx.x == 0) sh.cnt[0][0][0] = carry;
                __syncthreads();
                BPROF(5)
        };
        const bool scan = P.scanDecode != 0 || sh.scan != 0;
        if (!scan) {
            /*
             * Decode from the sweep's candidate lists (a few cells per diagonal instead of the whole
             * band): every wave walks its own list twice.  First the cells whose exponent reaches
             * logThrSlack are marked in the (diagonal, wave) masks (the exact threshold test of
             * diagonalCalculationPosteriorMatchProbs is the readback's), then, with the per-diagonal
             * offsets known, each hit is ranked inside its diagonal and written.
             */
            const int nC = sh.cnt[1][wave][0];
            for (int i = threadIdx.x; i < nPost * SY_MSK; i += SY_P) msk[i] = 0ull;
            __syncthreads();
            for (int pass = 0; pass < 2; pass++) {
#pragma unroll 1
                for (int i = lane; i < nC; i += 64) {
                    const int2 kx = myKx[i];
                    const int k = kx.x, x = kx.y, t = tPost0 - k;
                    const double ee = myFb[i] - wtot[k / 10].total;
                    if (!(x >= 1 && x <= t - 1 && ee >= P.logThrSlack)) continue;
                    /* (a candidate by its exponent alone: the device's exp() can come out an ulp below the host's, and
                     * the exact threshold test is the readback's, with the host libm) */
                    double p = exp(ee);
                    if (!pass) {
                        atomicOr(msk + k * (long long) SY_MSK + wave, 1ull << (x & 63));
                        continue;
                    }
                    /* rank inside the diagonal, as in the scan below */
                    const int xmin = bandTab[t].x;
                    const int W0 = SY_WAVE_OF(xmin), s0 = xmin & 63, c = SY_WMOD(wave - W0);
                    const unsigned long long fromS0 = ~0ull << s0, below = (1ull << lane) - 1ull;
                    const unsigned long long own = ld_msk(k * (long long) SY_MSK + wave);
                    int first = 0, beforeMine = 0, others = 0;
#pragma unroll
                    for (int w2 = 0; w2 < SY_R; w2++) {
                        const unsigned long long m2 = ld_msk(k * (long long) SY_MSK + w2);
                        const int c2 = SY_WMOD(w2 - W0);
                        if (c2 == 0) first = __popcll(m2 & fromS0);
                        else {
                            others += __popcll(m2);
                            if (c2 < c) beforeMine += __popcll(m2);
                        }
                    }
                    const int xl = x & 63;
                    const unsigned long long belowX = (1ull << xl) - 1ull;
                    int rank;
                    if (c != 0) rank = first + beforeMine + __popcll(own & belowX);
                    else if (xl >= s0) rank = __popcll(own & fromS0 & belowX);
                    else rank = first + others + __popcll(own & belowX);
                    const long long idx = out.nPairs + off[k] + rank;
                    if (idx < out.pairCap) {
                        if (p > 1.0) p = 1.0;
                        long long *o = out.pairs + idx * 3;
                        o[0] = (long long) floor(p * 10000000.0);
                        o[1] = x - 1;
                        o[2] = t - x - 1;
                        out.logp[idx] = ee;
                    }
                    (void) below;
                }
                if (!pass) { BPROF(3) } else { BPROF(6) }
                __syncthreads();
                if (!pass) { BPROF(4) } else { BPROF(7) }
                if (!pass) prefix();
            }
        } else
        for (int pass = 0; pass < 2; pass++) {
            int xs = wave * 64 + lane; /* this slot's k-mer: the one in (xmax-P, xmax] */
            {
                int a, b;
                band_load(bandTab, tPost0, a, b);
                xs += ((a - xs + SY_P - 1) / SY_P) * SY_P;
                if (xs > b) xs -= SY_P;
            }
            /* pass 1 works from the masks and offsets of a batch, fetched one batch ahead, one
             * (diagonal, wave) mask per lane 0..SY_MSK*U-1 and one offset per lane 0..U-1 */
            unsigned long long mvNext = 0ull;
            int ovNext = 0;
            /* the band of a batch's diagonals: one entry per lane 0..U-1, also a batch ahead */
            int2 bvNext = make_int2(1, 0);
            if (lane < SY_DECODE_U && lane < nPost) bvNext = bandTab[tPost0 - lane];
            if (pass) {
                const int kk = lane >> SY_MSK_SHIFT;
                if (lane < SY_MSK * SY_DECODE_U && kk < nPost) mvNext = ld_msk(kk * (long long) SY_MSK + (lane & (SY_MSK - 1)));
                if (lane < SY_DECODE_U && lane < nPost) ovNext = off[lane];
            }
#pragma unroll 1
            for (int k0 = 0; k0 < nPost; k0 += SY_DECODE_U) {
                const unsigned long long mv = mvNext;
                const int ov = ovNext;
                const int2 bv = bvNext;
                int xminA[SY_DECODE_U], xmaxA[SY_DECODE_U], xsA[SY_DECODE_U];
                double e[SY_DECODE_U], tot[SY_DECODE_U];
                unsigned long long own[SY_DECODE_U];
#pragma unroll
                for (int j = 0; j < SY_DECODE_U; j++) {
                    const int k = k0 + j, t = tPost0 - k;
                    const bool live = k < nPost;
                    xminA[j] = __builtin_amdgcn_readlane(bv.x, j);
                    xmaxA[j] = __builtin_amdgcn_readlane(bv.y, j);
                    if (live && xs > xmaxA[j]) xs -= SY_P;
                    xsA[j] = xs;
                    bool want = live && xs >= xminA[j];
                    own[j] = 0ull;
                    if (pass) {
                        own[j] = lane64(mv, j * SY_MSK + wave);
                        want = ((own[j] >> lane) & 1ull) != 0ull;
                    }
                    /* F.match + B.match, parked by the sweep in ring slot 3 */
                    const double *p = want ? g.rp(t, 3) : g.rw;
                    e[j] = *p;
                    tot[j] = wtot[(live ? k : 0) / 10].total;
                }
                {
                    const int ko = k0 + SY_DECODE_U + lane;
                    bvNext = make_int2(1, 0);
                    if (lane < SY_DECODE_U && ko < nPost) bvNext = bandTab[tPost0 - ko];
                }
                if (pass) {
                    const int kk = k0 + SY_DECODE_U + (lane >> SY_MSK_SHIFT), ko = k0 + SY_DECODE_U + lane;
                    mvNext = 0ull;
                    ovNext = 0;
                    if (lane < SY_MSK * SY_DECODE_U && kk < nPost) mvNext = ld_msk(kk * (long long) SY_MSK + (lane & (SY_MSK - 1)));
                    if (lane < SY_DECODE_U && ko < nPost) ovNext = off[ko];
                }
#pragma unroll
                for (int j = 0; j < SY_DECODE_U; j++) {
                    const int k = k0 + j, t = tPost0 - k, x = xsA[j];
                    const double ee = e[j] - tot[j];
                    if (!pass) {
                        if (k < nPost) {
                            const int xlo = xminA[j] > 1 ? xminA[j] : 1, xhi = xmaxA[j] < t - 1 ? xmaxA[j] : t - 1;
                            const bool ok = x >= xlo && x <= xhi && ee >= P.logThrSlack;
                            const unsigned long long m = __ballot(ok); /* (the exact threshold test is the readback's) */
                            if (lane == 0) msk[k * SY_MSK + wave] = m;
                        }
                    } else if (own[j] != 0ull) {
                        /* hits of this diagonal with a smaller k-mer index: the band starts in wave W0 at
                         * lane s0 and wraps around the waves, possibly back into W0's low lanes */
                        const int W0 = SY_WAVE_OF(xminA[j]), s0 = xminA[j] & 63;
                        const unsigned long long fromS0 = ~0ull << s0;
                        const int c = SY_WMOD(wave - W0);
                        int first = 0, beforeMine = 0, others = 0;
#pragma unroll
                        for (int w2 = 0; w2 < SY_R; w2++) {
                            const unsigned long long m2 = lane64(mv, j * SY_MSK + w2);
                            const int c2 = SY_WMOD(w2 - W0);
                            if (c2 == 0) first = __popcll(m2 & fromS0);
                            else {
                                others += __popcll(m2);
                                if (c2 < c) beforeMine += __popcll(m2);
                            }
                        }
                        const unsigned long long below = (1ull << lane) - 1ull;
                        int rank;
                        if (c != 0) rank = first + beforeMine + __popcll(own[j] & below);
                        else if (lane >= s0) rank = __popcll(own[j] & fromS0 & below);
                        else rank = first + others + __popcll(own[j] & below);
                        const long long idx = out.nPairs + __builtin_amdgcn_readlane(ov, j) + rank;
                        if (((own[j] >> lane) & 1ull) != 0ull && idx < out.pairCap) {
                            double p = exp(ee);
                            if (p > 1.0) p = 1.0;
                            long long *o = out.pairs + idx * 3;
                            o[0] = (long long) floor(p * 10000000.0);
                            o[1] = x - 1;
                            o[2] = t - x - 1;
                            out.logp[idx] = ee;
                        }
                    }
                }
            }
            if (!pass) { BPROF(3) } else { BPROF(6) }
            __syncthreads();
            if (!pass) { BPROF(4) } else { BPROF(7) }
            if (!pass) prefix();
        }
        out.nPairs += sh.cnt[0][0][0];
    }
    BPROF(8)
    BPROF_FLUSH
}

} // namespace

/* per-alignment scratch: [hit offsets | window totals | their terms | hit masks | candidate lists] */
static __host__ __device__ long long scratch_cand_offset(int ringD) {
    return 2ll * ringD * sizeof(int) + ((long long) ringD / 10 + 8) * (sizeof(WinTotal) + 2 * SY_P * sizeof(double))
           + (long long) SY_MSK * ringD * sizeof(unsigned long long);
}

static __host__ __device__ long long scratch_end_offset(int ringD) {
    return scratch_cand_offset(ringD) + (long long) SY_R * SY_CAND_PER_DIAG * ringD * (sizeof(int2) + sizeof(double));
}

/* One workgroup per alignment: forward sweep up to its next traceback point. */
extern "C" __global__ __launch_bounds__(SY_P) void SY_SYM(cpecan_k_sy_forward)(
    const DevItem *__restrict__ items, long long nItems, DevParams P,
    const int2 *__restrict__ bandTab, const double *__restrict__ track,
    const long long *__restrict__ trackBase, const double *__restrict__ events,
    const double *__restrict__ models, double *Fring, long long ringDoubles, int ringD,
    SyState *states) {
    __shared__ Shared sh;
    __shared__ Feed fd;
    __shared__ BandFeed bf;
    const long long idx = blockIdx.x;
    if (idx >= nItems) return;
    SyState *state = states + idx;
    const DevItem it = uniform_item(items[idx]);
    if (state->finished || it.lX + it.lY == 0) return;
    init_coef(sh.coef);
    __syncthreads();
    forward_window(it, P, bandTab + it.diagBase, track + trackBase[idx] * SY_ROW, events,
                   models + (long long) it.model * SY_MODEL_DOUBLES, Fring + idx * ringDoubles, ringD,
                   state, sh, fd, bf);
}

/* One workgroup per alignment: backward sweep + posterior decode of the window just described. */
extern "C" __global__ __launch_bounds__(SY_P) SY_BACKWARD_ATTR void SY_SYM(cpecan_k_sy_backward)(
    const DevItem *__restrict__ items, long long nItems, DevParams P,
    const int2 *__restrict__ bandTab, const double *__restrict__ track,
    const long long *__restrict__ trackBase, const double *__restrict__ models, double *Fring,
    long long ringDoubles, int ringD, SyState *states, long long *pairs, double *pairLogp,
    long long *totXay, double *totVal, char *scratch, long long scratchBytes, double *Bring, int window
#ifdef SY_FUSED
    , const unsigned short *__restrict__ kidx, double *expect
#endif
    ) {
    __shared__ Shared sh;
    __shared__ BandFeed bf;
#ifdef SY_VANILLA
    __shared__ TransFeed tf;
#endif
#ifdef SY_FX_LDS
    __shared__ double fxAcc[8 * SY_P];
#endif
    const long long idx = blockIdx.x;
    if (idx >= nItems) return;
    SyState *state = states + idx;
    if (!state->winValid) return;
    const DevItem it = uniform_item(items[idx]);
    init_coef(sh.coef);
    __syncthreads();
    ItemOut out;
    out.pairs = pairs + it.pairBase * 3;
    out.logp = pairLogp + it.pairBase;
    out.pairCap = it.pairCap;
    out.totXay = totXay + it.totBase;
    out.totVal = totVal + it.totBase;
    out.totCap = it.totCap;
    out.nPairs = uni64(state->nPairs);
    out.nTot = uni64(state->nTot);
    backward_window(it, P, bandTab + it.diagBase, track + trackBase[idx] * SY_ROW,
                    models + (long long) it.model * SY_MODEL_DOUBLES, Fring + idx * ringDoubles, ringD,
                    state, out, sh, bf, (int *) (scratch + idx * scratchBytes),
                    (WinTotal *) (scratch + idx * scratchBytes + 2ll * ringD * sizeof(int)),
                    (double *) (scratch + idx * scratchBytes + 2ll * ringD * sizeof(int)
                                + ((long long) ringD / 10 + 8) * sizeof(WinTotal)),
                    (unsigned long long *) (scratch + idx * scratchBytes + 2ll * ringD * sizeof(int)
                                            + ((long long) ringD / 10 + 8)
                                                  * (sizeof(WinTotal) + 2 * SY_P * sizeof(double))),
                    (int2 *) (scratch + idx * scratchBytes + scratch_cand_offset(ringD)),
                    (double *) (scratch + idx * scratchBytes + scratch_cand_offset(ringD)
                                + (long long) SY_R * SY_CAND_PER_DIAG * ringD * sizeof(int2)),
                    Bring ? Bring + idx * ((long long) ringD * SY_R * SY_BRING_VALUES * 64) : nullptr
#ifdef SY_VANILLA
                    , tf
#endif
#ifdef SY_FUSED
                    /* (DevParams::expectResweep: 1 every window down the second sweep, 2 those whose item and window
                     * parity differ) */
                    , fx_records(scratch + idx * scratchBytes + scratch_end_offset(ringD), ringD), expect, kidx,
                    P.expectResweep == 1 || (P.expectResweep == 2 && ((idx ^ window) & 1))
#ifdef SY_FX_LDS
                    , fxAcc
#endif
#ifdef SY_HDP_FUSED
                    , window
#endif
#endif
                    );
    if (threadIdx.x == 0) {
#ifndef SY_HDP_FUSED /* (the assignments were counted in place, as cpecan_k_sy_expect counts them) */
        state->nPairs = out.nPairs;
#endif
        state->nTot = out.nTot;
        state->winValid = 0;
        state->expectPending = SY_MODE(P) != 0 && !SY_FX ? window + 1 : 0; /* which launch's window the B ring holds */
    }
}

#if defined(SY_VANILLA) && !defined(SY_NO_ESTEP)
/*
 * The vanilla machine's expectations of the traceback window the backward kernel just swept (-DSY_VANILLA -DSY_ESTEP;
 * diagonalCalculation_Expectations :841-863 with cell_signal_updateBetaAndAlphaProb :478-498): of all transitions only
 * match -> gap X (into the skip bin of the cell's k-mer pair) and gap X -> gap X (bin + 30) are collected, both from the
 * cell's lower neighbour; the gap-X emission of this machine is 0.  The arithmetic of cpecan_k_wv_expect_v*
 * (cpecan_kernel_wave.hip), term for term, on this family's geometry: element-wise over the forward ring, the B ring
 * (B.gapX alone) and the window's exact totals, SY_EXPECT_CHUNKS workgroups to a window.  A thread keeps the two sums of
 * its column in registers and adds them to the column's bin (track row entry 21) when its slot moves on.
 */
extern "C" __global__ __launch_bounds__(SY_P) void SY_SYM(cpecan_k_sy_expect)(
    const DevItem *__restrict__ items, long long nItems, DevParams P, const int2 *__restrict__ bandTab,
    const double *__restrict__ track, const long long *__restrict__ trackBase,
    const unsigned short *__restrict__ kidx, const double *__restrict__ models, const double *Fring,
    long long ringDoubles, const double *Bring, int ringD, SyState *states, const char *scratch,
    long long scratchBytes, double *expect, int window) {
    __shared__ double sBins[64];
    (void) P; (void) kidx; (void) models;
    const long long idx = blockIdx.x;
    if (idx >= nItems) return;
    const SyState *state = states + idx;
    /* gridDim.y workgroups share a window's diagonals, a contiguous run each; the state record is only read here (the
     * backward kernel stamps it with the launch it belongs to) */
    if (state->expectPending != window + 1) return;
    const DevItem it = uniform_item(items[idx]);
    const Geometry g = make_geometry(const_cast<double *>(Fring) + idx * ringDoubles, ringD);
    const int lane = g.lane, wave = g.wave;
    const double *bown = Bring + idx * ((long long) ringD * SY_R * SY_BRING_VALUES * 64) + wave * (SY_BRING_VALUES * 64) + lane;
    const double *tr = track + trackBase[idx] * SY_ROW;
    const int2 *tab = bandTab + it.diagBase;
    const WinTotal *wtot = (const WinTotal *) (scratch + idx * scratchBytes + 2ll * ringD * sizeof(int));
    const int dTop = uni(state->winTop), from = uni(state->winFrom), to = uni(state->winTo);
    const int tPost0 = dTop < from ? dTop : from;
    double *dst = expect + (long long) it.model * CP_EXPECTV_LEN;
    if (threadIdx.x < 64) sBins[threadIdx.x] = 0.0;
    __syncthreads();

    double lik = 0.0, beta = 0.0, alpha = 0.0;
    int col = -1; /* matrix column whose sums beta / alpha hold */
    const int perChunk = (tPost0 - to + (int) gridDim.y - 1) / (int) gridDim.y;
    const int tHi = tPost0 - (int) blockIdx.y * perChunk;             /* this workgroup: diagonals tHi .. tLo+1 */
    const int tLo = tHi - perChunk > to ? tHi - perChunk : to;
    if (tHi > to) {
        int b0min, b0max, b1min, b1max;
        band_load(tab, tHi, b0min, b0max);
        int xs = wave * 64 + lane; /* this slot's k-mer: the one in (xmax-P, xmax] */
        xs += ((b0min - xs + SY_P - 1) / SY_P) * SY_P;
        if (xs > b0max) xs -= SY_P;
#pragma unroll 1
        for (int t = tHi; t > tLo; t--) {
            band_load(tab, t - 1, b1min, b1max);
            if (xs > b0max) xs -= SY_P;
            const int x = xs;
            const double total = wtot[(tPost0 - t) / 10].total;
            if (threadIdx.x == 0) lik += total;
            if (x >= b0min && x - 1 >= b1min && x - 1 <= b1max) { /* the cell (t, x) and its lower neighbour exist */
                const double Bx = bown[(long long) (t & g.ringMask) * (SY_R * SY_BRING_VALUES * 64)];
                const double l0 = *g.rpb(t - 1, 0), l1 = *g.rpb(t - 1, 1);
                const double *row = tr + (long long) x * SY_ROW;
                if (x != col) {
                    if (col >= 0) {
                        const int bin = (int) tr[(long long) col * SY_ROW + 21];
                        atomicAdd(&sBins[bin], beta);
                        atomicAdd(&sBins[bin + 30], alpha);
                    }
                    col = x;
                    beta = alpha = 0.0;
                }
                beta += exp(l0 + Bx + (0 + row[16]) - total);
                alpha += exp(l1 + Bx + (0 + row[17]) - total);
            }
            b0min = b1min; b0max = b1max;
        }
        if (col >= 0) {
            const int bin = (int) tr[(long long) col * SY_ROW + 21];
            atomicAdd(&sBins[bin], beta);
            atomicAdd(&sBins[bin + 30], alpha);
        }
    }
    __syncthreads();
    if (threadIdx.x < 60 && sBins[threadIdx.x] != 0.0) atomicAdd(dst + threadIdx.x, sBins[threadIdx.x]);
    if (threadIdx.x == 0 && lik != 0.0) atomicAdd(dst + 60, lik);
}
#endif

#if !defined(SY_NO_ESTEP) && !defined(SY_VANILLA) /* (the vanilla machine's E-step past 184 k-mers runs on the general
                    * kernel or on the _ve builds, in the form above; the HDP machine's past 248 k-mers on the general
                    * kernel or on the _he builds) */
/*
 * Baum-Welch expectations of the traceback window the backward kernel just swept
 * (diagonalCalculation_Expectations :841-863 with cell_signal_updateTransAndKmerSkipExpectations
 * :426-443).  By now every operand is in HBM -- forward cells and the two event-dependent emissions in
 * the forward ring, backward cells in the B ring, the window's exact totals in scratch -- so this is
 * an element-wise pass with no recurrence and no barrier: per cell eight exp(F.from + B.to + (eP + tP)
 * - total), summed per thread and reduced once per window.  A lane keeps the sum of its k-mer's
 * gap-X expectations in a register and adds it to the k-mer's bin when its slot moves to another k-mer.
 * The match block is skipped on the window's two lowest diagonals' worth of reach, as in the
 * reference, where forward[t-2] has been freed by then (quirk kept by the general kernel too).
 *
 * The HDP machine (-DSY_HDP -DSY_ESTEP; cell_signal_updateTransAndKmerSkipExpectations2 :445-476) collects the nine
 * transitions and the likelihood the same way, no k-mer bins, and an ASSIGNMENT for every transition into match whose
 * own posterior reaches the threshold: (from-state + 4 * window, x, y) with its exponent, appended to the alignment's
 * pair list in whatever order the threads of the window's workgroups get there (the host puts them into the
 * reference's order when it fetches them) -- the test and the record of cpecan_k_wv_expect_h*, expression for
 * expression.  Its transitions are the head of the DevHdpModel record, its gap-X emission the track's flat log(0.1).
 */
extern "C" __global__ __launch_bounds__(SY_P) void SY_SYM(cpecan_k_sy_expect)(
    const DevItem *__restrict__ items, long long nItems, DevParams P, const int2 *__restrict__ bandTab,
    const double *__restrict__ track, const long long *__restrict__ trackBase,
    const unsigned short *__restrict__ kidx, const double *__restrict__ models, const double *Fring,
    long long ringDoubles, const double *Bring, int ringD, SyState *states, const char *scratch,
    long long scratchBytes, double *expect, int window
#ifdef SY_HDP
    , long long *pairs, double *pairLogp
#endif
    ) {
    __shared__ double sExp[16];
    const long long idx = blockIdx.x;
    if (idx >= nItems) return;
    const SyState *state = states + idx;
    /* the pass has no recurrence: gridDim.y workgroups share a window's diagonals, a contiguous run each; the
     * state record is only read here (the backward kernel stamps it with the launch it belongs to) */
    if (state->expectPending != window + 1) return;
    const DevItem it = uniform_item(items[idx]);
#ifdef SY_HDP
    const double *model = ((const DevHdpModel *) models)[it.model].t;
    SyState *stateW = states + idx;
#else
    const double *model = models + (long long) it.model * CP_MODEL_STRIDE;
#endif
    double T[9];
#pragma unroll
    for (int i = 0; i < 9; i++) T[i] = model[i];
    const Geometry g = make_geometry(const_cast<double *>(Fring) + idx * ringDoubles, ringD);
    const int lane = g.lane, wave = g.wave;
    const double *bown = Bring + idx * ((long long) ringD * SY_R * 3 * 64) + wave * (3 * 64) + lane;
    const double *tr = track + trackBase[idx] * CP_ROW;
    const unsigned short *kx = kidx + it.xOff;
    const int2 *tab = bandTab + it.diagBase;
    const WinTotal *wtot = (const WinTotal *) (scratch + idx * scratchBytes + 2ll * ringD * sizeof(int));
    const int dTop = uni(state->winTop), from = uni(state->winFrom), to = uni(state->winTo);
    const int tPost0 = dTop < from ? dTop : from;
#ifdef SY_HDP
    double *dst = expect + (long long) it.model * (9 + 1);
#else
    double *dst = expect + (long long) it.model * (9 + 4096 + 1);
#endif

    double acc[8]; /* M>X X>X Y>X | M>M X>M Y>M | M>Y Y>Y */
#pragma unroll
    for (int i = 0; i < 8; i++) acc[i] = 0.0;
    double lik = 0.0, gapSum = 0.0;
    int gapX = -1; /* matrix column whose gap-X expectations gapSum holds */

    const int perChunk = (tPost0 - to + (int) gridDim.y - 1) / (int) gridDim.y;
    const int tHi = tPost0 - (int) blockIdx.y * perChunk;             /* this workgroup: diagonals tHi .. tLo+1 */
    const int tLo = tHi - perChunk > to ? tHi - perChunk : to;
    if (tHi <= to) return;
    int xs = wave * 64 + lane; /* this slot's k-mer: the one in (xmax-P, xmax] */
    int b0min, b0max, b1min, b1max, b2min, b2max;
    band_load(tab, tHi, b0min, b0max);
    band_load(tab, tHi - 1, b1min, b1max);
    xs += ((b0min - xs + SY_P - 1) / SY_P) * SY_P;
    if (xs > b0max) xs -= SY_P;
#pragma unroll 1
    for (int t = tHi; t > tLo; t--) {
        band_load(tab, t - 2, b2min, b2max);
        if (xs > b0max) xs -= SY_P;
        const int x = xs;
        const double total = wtot[(tPost0 - t) / 10].total;
        if (threadIdx.x == 0) lik += total;
        if (x >= b0min) { /* the cell (t, x) exists */
            const double *bc = bown + (long long) (t & g.ringMask) * (SY_R * 3 * 64);
            const double Bm = bc[0], Bx = bc[64], By = bc[128];
            const bool vLower = x - 1 >= b1min && x - 1 <= b1max;
            const bool vMiddle = t - 2 >= to && x - 1 >= b2min && x - 1 <= b2max;
            const bool vUpper = x >= b1min && x <= b1max;
            if (vLower) {
                const double l0 = *g.rpb(t - 1, 0), l1 = *g.rpb(t - 1, 1), l2 = *g.rpb(t - 1, 2);
                const double eP = tr[(long long) x * CP_ROW + CP_GAPX];
                const double p0 = exp(l0 + Bx + (eP + T[T_GAP_OPEN_X]) - total);
                const double p1 = exp(l1 + Bx + (eP + T[T_GAP_EXTEND_X]) - total);
                const double p2 = exp(l2 + Bx + (eP + T[T_GAP_SWITCH_TO_X]) - total);
                acc[0] += p0;
                acc[1] += p1;
                acc[2] += p2;
#ifndef SY_HDP
                if (x != gapX) {
                    if (gapX > 0) {
                        const int k = kx[gapX - 1];
                        if (k < 4096) atomicAdd(dst + 9 + k, gapSum);
                    }
                    gapX = x;
                    gapSum = 0.0;
                }
                gapSum += p0;
                gapSum += p1;
                gapSum += p2;
#endif
            }
            if (vMiddle) {
                const double m0 = *g.rpb(t - 2, 0), m1 = *g.rpb(t - 2, 1), m2 = *g.rpb(t - 2, 2);
                const double eP = *g.rp(t, 3);
#ifdef SY_HDP
                const double e0 = m0 + Bm + (eP + T[T_MATCH_CONTINUE]) - total;
                const double e1 = m1 + Bm + (eP + T[T_MATCH_FROM_GAP_X]) - total;
                const double e2 = m2 + Bm + (eP + T[T_MATCH_FROM_GAP_Y]) - total;
                const double q0 = exp(e0), q1 = exp(e1), q2 = exp(e2);
                acc[3] += q0;
                acc[4] += q1;
                acc[5] += q2;
                const double ee[3] = { e0, e1, e2 }, qq[3] = { q0, q1, q2 };
#pragma unroll
                for (int f = 0; f < 3; f++)
                    if (qq[f] >= P.threshold) {
                        const long long at = (long long) atomicAdd((unsigned long long *) &stateW->nPairs, 1ull);
                        if (at < it.pairCap) {
                            long long *o = pairs + (it.pairBase + at) * 3;
                            o[0] = f + 4ll * window;
                            o[1] = x - 1;
                            o[2] = (t - x) - 1;
                            pairLogp[it.pairBase + at] = ee[f];
                        }
                    }
#else
                acc[3] += exp(m0 + Bm + (eP + T[T_MATCH_CONTINUE]) - total);
                acc[4] += exp(m1 + Bm + (eP + T[T_MATCH_FROM_GAP_X]) - total);
                acc[5] += exp(m2 + Bm + (eP + T[T_MATCH_FROM_GAP_Y]) - total);
#endif
            }
            if (vUpper) {
                const double u0 = *g.rp(t - 1, 0), u2 = *g.rp(t - 1, 2);
                const double eP = *g.rp(t, 4);
                acc[6] += exp(u0 + By + (eP + T[T_GAP_OPEN_Y]) - total);
                acc[7] += exp(u2 + By + (eP + T[T_GAP_EXTEND_Y]) - total);
            }
        }
        b0min = b1min; b0max = b1max;
        b1min = b2min; b1max = b2max;
    }
#ifndef SY_HDP
    if (gapX > 0) {
        const int k = kx[gapX - 1];
        if (k < 4096) atomicAdd(dst + 9 + k, gapSum);
    }
#else
    (void) gapX; (void) gapSum; (void) kx;
#endif
    /* block reduction of the per-thread sums, then one atomic per value */
    if (threadIdx.x < 16) sExp[threadIdx.x] = 0.0;
    __syncthreads();
    const int slot[8] = { 0 * 3 + 1, 1 * 3 + 1, 2 * 3 + 1, 0 * 3 + 0, 1 * 3 + 0, 2 * 3 + 0, 0 * 3 + 2, 2 * 3 + 2 };
#pragma unroll
    for (int i = 0; i < 8; i++) {
        double v = acc[i];
        for (int o = 32; o > 0; o >>= 1) v += __shfl_down(v, o);
        if (lane == 0) atomicAdd(&sExp[slot[i]], v);
    }
    __syncthreads();
    if (threadIdx.x < 9) atomicAdd(dst + threadIdx.x, sExp[threadIdx.x]);
#ifdef SY_HDP
    if (threadIdx.x == 0) atomicAdd(dst + 9, lik);
#else
    if (threadIdx.x == 0) atomicAdd(dst + 9 + 4096, lik);
#endif
}
#endif /* !SY_NO_ESTEP && !SY_VANILLA */

#ifdef SY_PROFILE
extern "C" int SY_SYM(cpecan_systolic_prof_fetch)(unsigned long long *dst) {
    unsigned long long zero[SY_PROF_N] = {0};
    if (hipMemcpyFromSymbol(dst, HIP_SYMBOL(sy_prof), sizeof(zero)) != hipSuccess) return -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(sy_prof), zero, sizeof(zero)) == hipSuccess ? 0 : -1;
}
#endif
/* HBM scratch per alignment: a hit count and an output offset per ring diagonal, and per refresh of the window one
 * WinTotal and the two rows of per-cell terms */
static long long sy_scratch_bytes(int ringD) {
    return scratch_end_offset(ringD);
}

/* Launchers of the per-window stages of one pass over a batch (the C-ABI layer sequences them: the machine's track
 * (cpecan_kernel_prep.hip), then per window {forward, backward}, then its counts). */
static int sy_status() { return hipGetLastError() == hipSuccess ? 0 : -1; }
static int sy_launch_forward(hipStream_t stream, const SweepArgs &a, int) {
    hipLaunchKernelGGL(SY_SYM(cpecan_k_sy_forward), dim3((unsigned) a.nItems), dim3(SY_P), 0, stream, a.items, a.nItems,
                       a.P, a.bandTab, a.track, a.trackBase, a.events, a.models, a.Fring, a.ringDoubles, a.ringD,
                       (SyState *) a.states);
    return sy_status();
}
static int sy_launch_backward(hipStream_t stream, const SweepArgs &a, int window) {
    hipLaunchKernelGGL(SY_SYM(cpecan_k_sy_backward), dim3((unsigned) a.nItems), dim3(SY_P), 0, stream, a.items, a.nItems,
                       a.P, a.bandTab, a.track, a.trackBase, a.models, a.Fring, a.ringDoubles, a.ringD,
                       (SyState *) a.states, a.pairs, a.pairLogp, a.totXay, a.totVal, a.scratch, a.scratchBytes, a.Bring,
                       window
#ifdef SY_FUSED
                       , a.kidx, a.expect
#endif
                       );
    return sy_status();
}
#ifndef SY_NO_ESTEP
static int sy_launch_expect(hipStream_t stream, const SweepArgs &a, int window) {
    hipLaunchKernelGGL(SY_SYM(cpecan_k_sy_expect), dim3((unsigned) a.nItems, SY_EXPECT_CHUNKS), dim3(SY_P), 0, stream,
                       a.items, a.nItems, a.P, a.bandTab, a.track, a.trackBase, a.kidx, a.models, a.Fring, a.ringDoubles,
                       a.Bring, a.ringD, (SyState *) a.states, a.scratch, a.scratchBytes, a.expect, window
#ifdef SY_HDP
                       , a.pairs, a.pairLogp
#endif
                       );
    return sy_status();
}
#endif

/* the record (host only: the device pass would emit it as a constant, with pointers to host functions) */
#ifndef __HIP_DEVICE_COMPILE__
#define SY_BUILD_SYM SY_SYM(cpecan_systolic_build)
extern "C" const SweepBuild SY_BUILD_SYM;
/* (the _f builds serve a batch that asks for them only: cpecan_hip.hip puts one in the place of the build of as many
 * waves that the dispatch chose; their segment records lie behind the scratch.  The dispatch sends the other E-step
 * builds of the vanilla and the HDP machine no posterior batch, and their posterior builds no E-step) */
const SweepBuild SY_BUILD_SYM = {
    SY_R, false, SY_MACHINE_ID, &SY_MACHINE, SY_P - 2 * SY_PREFETCH, SY_R * SY_RING_VALUES * 64, SY_BRING_ROW_DOUBLES,
    sy_scratch_bytes, SY_ESTEP_BY(sy_fx_bytes, nullptr), sy_launch_forward, sy_launch_backward,
    SY_ESTEP_BY(sy_launch_backward, nullptr), SY_ESTEP_BY(nullptr, sy_launch_expect), nullptr };
#endif
