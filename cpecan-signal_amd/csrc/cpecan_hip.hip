/*
 * cpecan_hip.hip -- the C-ABI of include/cpecan_hip.h: contexts, the kernel choice (choose_dispatch, and the plan calls
 * that ask it without a device) and batches from creation to destruction (the model tables: cpecan_models.hip; how a run
 * is queued: cpecan_run.hip; what a finished run gives back: cpecan_readback.hip).
 *
 * Host side of the thin layer between the reference-shaped C host code and the gfx950 kernels.
 * Nothing here computes DP cells: when no GPU is usable every compute entry point fails with
 * CPECAN_ENODEVICE (there is deliberately no CPU fallback).
 */
#include "cpecan_band_extent.h"
#include "cpecan_batch.h"

#include "cpecan_sweep.h"

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdarg>
#include <cstring>
#include <new>
#include <sched.h>
#include <thread>

extern "C" __global__ void cpecan_k_general(DevGeneralArgs, DevParams);
extern "C" __global__ void cpecan_k_general4(DevGeneralArgs, DevParams);
extern "C" __global__ void cpecan_k_general5(DevGeneralArgs, DevParams);
extern "C" __global__ void cpecan_k_generalv(DevGeneralArgs, DevParams);
extern "C" __global__ void cpecan_k_generalh(DevGeneralArgs, DevParams);

/* The builds of the throughput kernels (SweepBuild, cpecan_sweep.h), each defined next to its kernels.  Which builds
 * exist, and what each is compiled with, is the Makefile's list (SY_BUILDS, WV_BUILDS: make print-builds); the
 * declarations and tables below say which build serves which band.
 * A family's table is indexed by the rows a band of that width asks for, minus one: the workgroup family with 1..4 waves
 * per workgroup (bands up to 56, 120, 184, 248 k-mers; the narrower the band, the more alignments are resident per CU),
 * the wave family with 2..4 cells per lane (a one-cell build would only serve bands below 57 k-mers, which the two-cell
 * build takes too; the vanilla machine has no four-cell build, it spills: its bands above 184 k-mers run on the general
 * kernel).  A table of wide builds (six and eight waves per workgroup: bands up to 376 and 504 k-mers; the vanilla
 * tables start at four waves, because the vanilla wave builds end at 184) is reached only when the batch's widest band
 * is past every build of the tables above and the batch carries the table's flag: CPECAN_FLAG_WIDE_BANDS for the
 * strawMan machine (_r) and the vanilla machine's posterior decode (_v), CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP for the
 * vanilla E-step (_ve; without it that E-step stays on the general kernel), CPECAN_FLAG_WIDE_BANDS_HDP for the HDP
 * machine's posterior decode (_h), CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP for its E-step (_he).  The fused builds (_f, _vf, _hf
 * of either family: the E-step summed inside the sweep back, and no other form of it) are in no table here: each stands
 * in for the build of as many rows that the rules above come to, as the last step of choose_dispatch and for a batch of
 * expectations alone (FUSED_STAND_INS, which also says what asks for each). */
#define SWEEP_BUILD(name) extern "C" const SweepBuild name;
SWEEP_BUILD(cpecan_systolic_build_r1) SWEEP_BUILD(cpecan_systolic_build_r2) SWEEP_BUILD(cpecan_systolic_build_r3)
SWEEP_BUILD(cpecan_systolic_build) SWEEP_BUILD(cpecan_systolic_build_r6) SWEEP_BUILD(cpecan_systolic_build_r8)
SWEEP_BUILD(cpecan_wave_build_l2) SWEEP_BUILD(cpecan_wave_build_l3) SWEEP_BUILD(cpecan_wave_build_l4)
SWEEP_BUILD(cpecan_wave_build_h2) SWEEP_BUILD(cpecan_wave_build_h3) SWEEP_BUILD(cpecan_wave_build_h4)
SWEEP_BUILD(cpecan_wave_build_v2) SWEEP_BUILD(cpecan_wave_build_v3)
SWEEP_BUILD(cpecan_wave_build_vf2) SWEEP_BUILD(cpecan_wave_build_vf3)
SWEEP_BUILD(cpecan_wave_build_hf2) SWEEP_BUILD(cpecan_wave_build_hf3) SWEEP_BUILD(cpecan_wave_build_hf4)
SWEEP_BUILD(cpecan_systolic_build_v4) SWEEP_BUILD(cpecan_systolic_build_v6) SWEEP_BUILD(cpecan_systolic_build_v8)
SWEEP_BUILD(cpecan_systolic_build_h6) SWEEP_BUILD(cpecan_systolic_build_h8)
SWEEP_BUILD(cpecan_systolic_build_he6) SWEEP_BUILD(cpecan_systolic_build_he8)
SWEEP_BUILD(cpecan_systolic_build_ve4) SWEEP_BUILD(cpecan_systolic_build_ve6) SWEEP_BUILD(cpecan_systolic_build_ve8)
SWEEP_BUILD(cpecan_systolic_build_f1) SWEEP_BUILD(cpecan_systolic_build_f2) SWEEP_BUILD(cpecan_systolic_build_f3)
SWEEP_BUILD(cpecan_systolic_build_f4) SWEEP_BUILD(cpecan_systolic_build_f6) SWEEP_BUILD(cpecan_systolic_build_f8)
SWEEP_BUILD(cpecan_systolic_build_vf4) SWEEP_BUILD(cpecan_systolic_build_vf6) SWEEP_BUILD(cpecan_systolic_build_vf8)
SWEEP_BUILD(cpecan_systolic_build_hf6) SWEEP_BUILD(cpecan_systolic_build_hf8)
static SweepFamily SY_BUILDS = { &cpecan_systolic_build_r1, &cpecan_systolic_build_r2, &cpecan_systolic_build_r3,
                                 &cpecan_systolic_build };
/* (a table of wide builds ends with a null entry) */
static const SweepBuild *const SY_WIDE_BUILDS[3] = { &cpecan_systolic_build_r6, &cpecan_systolic_build_r8, nullptr };
static const SweepBuild *const SYV_WIDE_BUILDS[4] = { &cpecan_systolic_build_v4, &cpecan_systolic_build_v6,
                                                      &cpecan_systolic_build_v8, nullptr };
static const SweepBuild *const SYH_WIDE_BUILDS[3] = { &cpecan_systolic_build_h6, &cpecan_systolic_build_h8, nullptr };
static const SweepBuild *const SYHE_WIDE_BUILDS[3] = { &cpecan_systolic_build_he6, &cpecan_systolic_build_he8, nullptr };
static const SweepBuild *const SYVE_WIDE_BUILDS[4] = { &cpecan_systolic_build_ve4, &cpecan_systolic_build_ve6,
                                                       &cpecan_systolic_build_ve8, nullptr };
static SweepFamily WV_BUILDS = { &cpecan_wave_build_l2, &cpecan_wave_build_l2, &cpecan_wave_build_l3, &cpecan_wave_build_l4 };
static SweepFamily HV_BUILDS = { &cpecan_wave_build_h2, &cpecan_wave_build_h2, &cpecan_wave_build_h3, &cpecan_wave_build_h4 };
static SweepFamily VV_BUILDS = { &cpecan_wave_build_v2, &cpecan_wave_build_v2, &cpecan_wave_build_v3, &cpecan_wave_build_v3 };

namespace {

thread_local std::string g_err;

/* std::vector without the zero-fill of resize(): the big host tables here are written in full right after they are
 * sized (by several threads, so the page faults spread too) */
template <class T> struct NoInit : std::allocator<T> {
    template <class U> struct rebind { using other = NoInit<U>; };
    template <class U, class... A> void construct(U *p, A &&...a) {
        if constexpr (sizeof...(A) == 0) ::new ((void *) p) U;
        else ::new ((void *) p) U(std::forward<A>(a)...);
    }
};

} // namespace

/* worker threads for host-side table derivation: the CPUs this process may run on (its affinity mask, which is
 * what a job's CPU share shows up as), at most 32 -- a node's hardware_concurrency() is the whole machine, and
 * eight ranks of a multi-GPU job each spawning that many threads would run into the host's task limits */
int host_threads() {
    int n = (int) std::thread::hardware_concurrency();
    cpu_set_t set;
    if (sched_getaffinity(0, sizeof set, &set) == 0) {
        const int c = CPU_COUNT(&set);
        if (c > 0 && c < n) n = c;
    }
    return n < 1 ? 1 : n > 32 ? 32 : n;
}

/* what the calling thread's last DevBuf allocation was refused for by an account's limit (asked < 0: nothing) */
static thread_local struct { long long asked = -1, limit = 0, live = 0; } g_memRefused;

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    if (code == CPECAN_EHIP && g_memRefused.asked >= 0) { /* the hipErrorOutOfMemory was the account's, not the device's */
        snprintf(buf, sizeof buf, "device memory limit of the context: %lld bytes asked for, limit %lld bytes (%lld held)",
                 g_memRefused.asked, g_memRefused.limit, g_memRefused.live);
        g_err = buf;
        code = CPECAN_ELIMIT;
    }
    g_memRefused.asked = -1;
    return code;
}

std::shared_ptr<MemAccount> &mem_current() {
    static thread_local std::shared_ptr<MemAccount> a;
    return a;
}
MemScope::MemScope(const std::shared_ptr<MemAccount> &a) : outer(mem_current()) {
    mem_current() = a;
    g_memRefused.asked = -1;
}
MemScope::~MemScope() {
    mem_current() = outer;
    g_memRefused.asked = -1; /* (a refusal that nobody reported must not colour a later call's failure) */
}
void mem_refused(size_t asked, const MemAccount &a) {
    g_memRefused.asked = (long long) asked;
    g_memRefused.limit = a.limit;
    g_memRefused.live = a.live;
}

DevCache &dev_cache() {
    static DevCache *c = new DevCache(false); /* (never destroyed: the runtime may be gone by the time statics are) */
    return *c;
}
DevCache &pinned_cache() {
    static DevCache *c = new DevCache(true);
    return *c;
}

#define NO_WIDE { nullptr, 0 }
const MachineRow MACHINES[N_MACHINES] = {
    /* STRAWMAN */ { 3, CPECAN_EXPECTATION_LEN, 4, 0, nullptr, nullptr, false, &WV_BUILDS, &SY_BUILDS,
                     { { SY_WIDE_BUILDS, CPECAN_FLAG_WIDE_BANDS }, { SY_WIDE_BUILDS, CPECAN_FLAG_WIDE_BANDS } }, false, cpecan_k_general, X_KIDX, false, 0 },
    /* DNA5 */     { 5, CPECAN_EXPECTATION5_LEN, 4, 0, nullptr, "DNA batches: no cell dumps", true, nullptr, nullptr, { NO_WIDE, NO_WIDE },
                     false, cpecan_k_general5, X_CHARS, false, 248 },
    /* VANILLA */  { 3, CPECAN_EXPECTATIONV_LEN, 4, 0, nullptr, "vanilla batches: no cell dumps", true, &VV_BUILDS, nullptr,
                     { { SYV_WIDE_BUILDS, CPECAN_FLAG_WIDE_BANDS }, { SYVE_WIDE_BUILDS, CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP } }, true,
                     cpecan_k_generalv, X_KIDX, true, 0 },
    /* HDP */      { 3, CPECAN_EXPECTATIONH_LEN, 16, 0, nullptr, "HDP batches: no cell dumps", true, &HV_BUILDS, nullptr,
                     { { SYH_WIDE_BUILDS, CPECAN_FLAG_WIDE_BANDS_HDP }, { SYHE_WIDE_BUILDS, CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP } }, true,
                     cpecan_k_generalh, X_KID, false, 0 },
    /* SM4 */      { 4, CPECAN_EXPECTATION_LEN, 4, 0, "4-state batches: posterior decode only, no cell dumps",
                     "4-state batches: posterior decode only, no cell dumps", false, nullptr, nullptr, { NO_WIDE, NO_WIDE }, false,
                     cpecan_k_general4, X_KIDX, false, 0 },
    /* ECHELON */  { 7, CPECAN_EXPECTATION_LEN, 16, 4, "echelon batches: posterior decode only, no cell dumps",
                     "echelon batches: posterior decode only, no cell dumps", false, nullptr, nullptr, { NO_WIDE, NO_WIDE }, false,
                     nullptr, X_KIDX, true, 0 },
};

/* what a machine refuses whatever the batch holds */
static int check_machine(Machine machine, int mode, int flags) {
    const MachineRow &m = MACHINES[machine];
    if (mode != CPECAN_MODE_POSTERIOR && mode != CPECAN_MODE_EXPECTATIONS) return fail(CPECAN_EINVAL, "unknown mode %d", mode);
    if (m.posteriorOnly && mode != CPECAN_MODE_POSTERIOR) return fail(CPECAN_EINVAL, "%s", m.posteriorOnly);
    if (m.noDumps && (flags & CPECAN_FLAG_DEBUG_DUMP)) return fail(CPECAN_EINVAL, "%s", m.noDumps);
    if (m.bandedEstep && mode == CPECAN_MODE_EXPECTATIONS && (flags & CPECAN_FLAG_UNBANDED))
        return fail(CPECAN_EINVAL, "expectations run over the banded matrix only");
    return CPECAN_OK;
}

/* The environment switches that change what a batch runs on or how its storage is sized, parsed once per batch (tests
 * and timing tools set them between batches); CPECAN_DNA_GENERAL once per process.  Nothing else between
 * batch_create_impl and index_kmers reads the environment for such a switch (what is left there: diagnostics). */
struct BatchEnv {
    int wideFlags;    /* the wide-band flags whose variable is 1, for every batch whose machine and mode have wide builds
                         behind that flag: CPECAN_WIDE_BANDS (CPECAN_FLAG_WIDE_BANDS), CPECAN_WIDE_BANDS_HDP (.._HDP: HDP
                         posterior batches), CPECAN_WIDE_BANDS_HDP_ESTEP (.._HDP_ESTEP: HDP batches of expectations),
                         CPECAN_WIDE_BANDS_VANILLA_ESTEP (.._VANILLA_ESTEP: vanilla batches of expectations) */
    bool waveKernels; /* false under CPECAN_KERNELS=systolic: the workgroup-per-alignment family for every batch */
    int systolicRows; /* CPECAN_SYSTOLIC_ROWS=N: a build of at least N rows (tests, timing) */
    int asmMode;      /* CPECAN_ASM: 0 the compiled kernels, 1 the assembly forward sweep only (the compiled sweep back
                         reads what it writes), otherwise and unset (-1) both assembly sweeps (tests, timing) */
    bool wave5Off;    /* CPECAN_DNA_GENERAL: the 5-state machine on the general kernel (tests, timing) */
    bool asmNarrow;   /* CPECAN_ASM_NARROW=1: CPECAN_FLAG_ASM_NARROW_BANDS for every batch it means something to */
    bool fusedWorkgroup, fusedWide; /* CPECAN_EXPECT_FUSED_WORKGROUP=1, CPECAN_EXPECT_FUSED_WIDE=1: CPECAN_FLAG_WORKGROUP_FUSED_ESTEP,
                                       CPECAN_FLAG_WIDE_BANDS_FUSED_ESTEP for every batch they mean something to */
    bool ringEstep;      /* CPECAN_EXPECT_FUSED=0: the E-step from the ring of backward cells on the builds that have both forms */
    int expectResweep;   /* CPECAN_EXPECT_RESWEEP, for a fused E-step (DevParams::expectResweep; unset: 0) */
    int systolicGroups;  /* CPECAN_SYSTOLIC_GROUPS: the stream groups of a batch, 1..8 (0, unset: the family's own number) */
    long long ringPad;   /* CPECAN_RING_PAD: doubles added to every alignment's ring (tests; unset: 0) */
};
static BatchEnv read_batch_env() {
    static const bool wave5Off = getenv("CPECAN_DNA_GENERAL") != nullptr;
    const char *wide = getenv("CPECAN_WIDE_BANDS"), *kernels = getenv("CPECAN_KERNELS");
    const char *rows = getenv("CPECAN_SYSTOLIC_ROWS"), *as = getenv("CPECAN_ASM"), *wideH = getenv("CPECAN_WIDE_BANDS_HDP");
    const char *wideHE = getenv("CPECAN_WIDE_BANDS_HDP_ESTEP"), *wideVE = getenv("CPECAN_WIDE_BANDS_VANILLA_ESTEP");
    const char *narrow = getenv("CPECAN_ASM_NARROW");
    const char *fxw = getenv("CPECAN_EXPECT_FUSED_WORKGROUP"), *fxd = getenv("CPECAN_EXPECT_FUSED_WIDE");
    const char *fx = getenv("CPECAN_EXPECT_FUSED"), *resweep = getenv("CPECAN_EXPECT_RESWEEP");
    const char *groups = getenv("CPECAN_SYSTOLIC_GROUPS"), *pad = getenv("CPECAN_RING_PAD");
    const int wideFlags = (wide && atoi(wide) == 1 ? CPECAN_FLAG_WIDE_BANDS : 0) |
                          (wideH && atoi(wideH) == 1 ? CPECAN_FLAG_WIDE_BANDS_HDP : 0) |
                          (wideHE && atoi(wideHE) == 1 ? CPECAN_FLAG_WIDE_BANDS_HDP_ESTEP : 0) |
                          (wideVE && atoi(wideVE) == 1 ? CPECAN_FLAG_WIDE_BANDS_VANILLA_ESTEP : 0);
    return { wideFlags, !(kernels && strcmp(kernels, "systolic") == 0), rows ? atoi(rows) : 1, as ? atoi(as) : -1, wave5Off,
             narrow != nullptr && atoi(narrow) == 1, fxw != nullptr && atoi(fxw) == 1, fxd != nullptr && atoi(fxd) == 1,
             fx != nullptr && atoi(fx) == 0, resweep ? atoi(resweep) : 0,
             groups ? std::min(std::max(atoi(groups), 1), 8) : 0, pad ? atoll(pad) : 0 };
}

/* The kernel choice: a function of the machine, what the caller asked for, the environment, two facts about the
 * batch's bands and one about its characters (a vanilla batch that meets a k-mer that is none).  Asked about the narrowest band there is (maxWidth 0, edges stepping by one) it tells what holds
 * for every band: what it refuses then, it refuses always, and the general kernel then is the general kernel always. */
struct DispatchQuery {
    Machine machine;
    int mode, kernel, flags;
    int maxWidth;        /* the widest band of the batch, in cells */
    bool edgesStepByOne; /* every band edge moves by at most one k-mer per diagonal */
    BatchEnv env;
    bool noKmer = false; /* a vanilla item meets a k-mer that is none (vanilla_meets_no_kmer) */
};
struct Dispatch {
    int kernel = CPECAN_KERNEL_GENERAL; /* CPECAN_KERNEL_GENERAL or _SYSTOLIC, as cpecan_hip_batch_info reports */
    const SweepBuild *build = nullptr;  /* the build the batch runs on (null on the general kernel) */
    bool fused = false;     /* an E-step that sums its expectations inside the sweep back: no ring of backward cells, no
                               expectation kernel (cpecan_hip_batch_expectation_pass) */
    int expectResweep = 0;  /* ... and its DevParams::expectResweep */
    bool wave5 = false;     /* the 5-state machine's wave kernels (cpecan_kernel_wave5.hip) in place of the general one */
    bool wave4 = false;     /* the 4-state machine's wave kernels (cpecan_kernel_wave4.hip) in place of the general one */
    bool asmPlan = false;   /* the hand-scheduled assembly sweeps may take the batch, as far as the bands do not matter */
    bool asmSweeps = false; /* ... and with its bands; what is left is known at set-up (one stream group, the module) */
    bool asmBackward = false; /* ... both sweeps (CPECAN_ASM=1: the forward sweep only) */
    int asmCells = 0;       /* cells per lane of the assembly sweeps that take it (asmSweeps): ASM_L or ASM2_L */
    int flags = 0;          /* the batch's flags (CPECAN_WIDE_BANDS=1 adds its flag where it means something) */
    int refusal = CPECAN_OK;
    char why[160] = "";
};
/* The fused builds: a batch of expectations that the rules of choose_dispatch put on a row's ring build, and that carries
 * the row's flag or whose environment has the row's switch on, runs on the row's fused build, of as many waves per
 * workgroup or cells per lane.  A ring build belongs to one machine, one family and one range of bands, and a flag is on
 * the rows of its own builds alone: to any other batch (another machine, mode, family or range of bands, the general
 * kernel) it means nothing, and that batch runs what it runs without it -- so the flag of _h2 / _h3 moves no batch off
 * _h4, and a wave build's flag none off the _ve / _he workgroup builds: those rows have flags of their own. */
static const struct FusedStandIn {
    const SweepBuild *ring, *fused;
    int flag;
    bool BatchEnv::*env; /* (null: no variable) */
} FUSED_STAND_INS[] = {
    { &cpecan_systolic_build_r1, &cpecan_systolic_build_f1, CPECAN_FLAG_WORKGROUP_FUSED_ESTEP, &BatchEnv::fusedWorkgroup },
    { &cpecan_systolic_build_r2, &cpecan_systolic_build_f2, CPECAN_FLAG_WORKGROUP_FUSED_ESTEP, &BatchEnv::fusedWorkgroup },
    { &cpecan_systolic_build_r3, &cpecan_systolic_build_f3, CPECAN_FLAG_WORKGROUP_FUSED_ESTEP, &BatchEnv::fusedWorkgroup },
    { &cpecan_systolic_build, &cpecan_systolic_build_f4, CPECAN_FLAG_WORKGROUP_FUSED_ESTEP, &BatchEnv::fusedWorkgroup },
    { &cpecan_systolic_build_r6, &cpecan_systolic_build_f6, CPECAN_FLAG_WIDE_BANDS_FUSED_ESTEP, &BatchEnv::fusedWide },
    { &cpecan_systolic_build_r8, &cpecan_systolic_build_f8, CPECAN_FLAG_WIDE_BANDS_FUSED_ESTEP, &BatchEnv::fusedWide },
    { &cpecan_wave_build_v2, &cpecan_wave_build_vf2, CPECAN_FLAG_VANILLA_FUSED_ESTEP, nullptr },
    { &cpecan_wave_build_v3, &cpecan_wave_build_vf3, CPECAN_FLAG_VANILLA_FUSED_ESTEP, nullptr },
    { &cpecan_wave_build_h2, &cpecan_wave_build_hf2, CPECAN_FLAG_HDP_FUSED_ESTEP, nullptr },
    { &cpecan_wave_build_h3, &cpecan_wave_build_hf3, CPECAN_FLAG_HDP_FUSED_ESTEP, nullptr },
    { &cpecan_wave_build_h4, &cpecan_wave_build_hf4, CPECAN_FLAG_HDP_FOUR_CELLS_FUSED_ESTEP, nullptr },
    { &cpecan_systolic_build_ve4, &cpecan_systolic_build_vf4, CPECAN_FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP, nullptr },
    { &cpecan_systolic_build_ve6, &cpecan_systolic_build_vf6, CPECAN_FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP, nullptr },
    { &cpecan_systolic_build_ve8, &cpecan_systolic_build_vf8, CPECAN_FLAG_WIDE_BANDS_VANILLA_FUSED_ESTEP, nullptr },
    { &cpecan_systolic_build_he6, &cpecan_systolic_build_hf6, CPECAN_FLAG_WIDE_BANDS_HDP_FUSED_ESTEP, nullptr },
    { &cpecan_systolic_build_he8, &cpecan_systolic_build_hf8, CPECAN_FLAG_WIDE_BANDS_HDP_FUSED_ESTEP, nullptr },
};
#define CP_WAVE5_MAX_WIDTH 192 /* cells: one to three per lane */
#define CP_WAVE4_MAX_WIDTH 128 /* cells: one or two per lane */
static Dispatch choose_dispatch(const DispatchQuery &q) {
    const MachineRow &m = MACHINES[q.machine];
    const bool unbanded = (q.flags & CPECAN_FLAG_UNBANDED) != 0, debug = (q.flags & CPECAN_FLAG_DEBUG_DUMP) != 0;
    Dispatch d;
    d.flags = q.flags;
    auto refuse = [&d](const char *fmt, int a = 0, int b = 0) {
        d.refusal = CPECAN_EINVAL;
        snprintf(d.why, sizeof d.why, fmt, a, b);
        return d;
    };
    /* the HDP and vanilla machines have wave-per-alignment kernels of their own, for the posterior decode and for the
     * E-step, and CPECAN_FLAG_GENERAL_KERNEL keeps such a batch on the general kernel; the 5-state, 4-state and
     * echelon machines have none among the sweep builds (the one-wave kernels of the first two are chosen at the end) */
    /* the reference scores a k-mer that is none as NaN under the vanilla machine, and NaN spreads through its logAdd;
     * cpecan_k_generalv adds as the reference does, the register-resident kernels' branch-free logAdd (v_max / v_min)
     * drops a NaN operand: such a batch runs on the general kernel */
    const int asked = !m.wave || (q.machine == VANILLA && q.noKmer) ? CPECAN_KERNEL_GENERAL
                      : !m.ownChoice ? q.kernel
                      : (q.flags & CPECAN_FLAG_GENERAL_KERNEL) ? CPECAN_KERNEL_GENERAL : CPECAN_KERNEL_AUTO;
    if (unbanded && (q.mode != CPECAN_MODE_POSTERIOR || asked == CPECAN_KERNEL_SYSTOLIC))
        return refuse("un-banded alignment: posterior mode on the general kernel only");
    /* the wide builds of the workgroup family are the strawMan machine's, the HDP machine's and the vanilla machine's.
     * A machine's wide builds of a mode answer to the flag its row names for that mode (the HDP machine's to two of its
     * own, one per mode; the vanilla machine's E-step to one of its own) and each flag has its environment variable: a
     * flag means nothing to the machines and modes of another flag or of none -- a vanilla E-step past the wave builds
     * runs on the general kernel whatever the other three flags say */
    const MachineRow::Wide &wide = m.wide[q.mode];
    const bool wideServes = wide.builds != nullptr;
    if (wideServes) d.flags |= wide.flag & q.env.wideFlags;
    if (asked != CPECAN_KERNEL_GENERAL) {
        /* the family the batch would run on, and the widest band its builds take */
        const bool workgroup = m.workgroup && (!q.env.waveKernels || (q.flags & CPECAN_FLAG_WORKGROUP_KERNELS));
        const SweepFamily &fam = workgroup ? *m.workgroup : *m.wave;
        /* the machine's wide-bands flag: a band past the family's widest build goes to the narrowest wide build of the
         * workgroup family that holds it (six or eight waves; four, six or eight for the vanilla machine, in either
         * mode), whichever family the batch would otherwise run on; a band the family holds is left to it */
        const SweepBuild *wideBuild = nullptr;
        int reach = fam[3]->maxWidth;
        if (wideServes && (d.flags & wide.flag))
            for (int i = 0; wide.builds[i] != nullptr; i++) {
                if (!wideBuild && q.maxWidth > fam[3]->maxWidth && q.maxWidth <= wide.builds[i]->maxWidth) wideBuild = wide.builds[i];
                reach = std::max(reach, wide.builds[i]->maxWidth);
            }
        const bool fits = q.maxWidth <= reach && q.edgesStepByOne;
        d.kernel = asked != CPECAN_KERNEL_AUTO ? asked
                   : fits && !debug && !unbanded ? CPECAN_KERNEL_SYSTOLIC : CPECAN_KERNEL_GENERAL;
        if (d.kernel == CPECAN_KERNEL_SYSTOLIC && !fits)
            return refuse("band is %d cells wide (systolic kernel: at most %d, edges moving one k-mer per diagonal)",
                          q.maxWidth, reach);
        if (d.kernel == CPECAN_KERNEL_SYSTOLIC && debug) return refuse("cell dumps are only available from the general kernel");
        if (d.kernel == CPECAN_KERNEL_SYSTOLIC) {
            /* the build with the fewest waves per workgroup whose slots hold the widest band: the fewer waves an
             * alignment takes, the more alignments a CU holds */
            int r = q.env.systolicRows < 1 ? 1 : q.env.systolicRows > 4 ? 4 : q.env.systolicRows;
            while (r < 4 && q.maxWidth > fam[r - 1]->maxWidth) r++;
            d.build = wideBuild ? wideBuild : fam[r - 1];
            /* (the builds without an E-step are the wide builds of a machine's posterior mode) */
            if (q.mode == CPECAN_MODE_EXPECTATIONS && !d.build->expect && !d.build->backward_fx)
                return refuse("the chosen kernel build has no E-step");
            /* the assembly sweeps take the posterior batches of a family that has a build for them (the strawMan
             * machine's wave family) whose bands need ASM_L cells per lane and fit their staging scheme -- and, for a
             * batch that asked for it (CPECAN_FLAG_ASM_NARROW_BANDS, CPECAN_ASM_NARROW=1), those whose bands need
             * ASM2_L: both sweeps at two cells per lane */
            d.asmPlan = q.mode == CPECAN_MODE_POSTERIOR && fam[ASM_L - 1]->post_asm != nullptr;
            d.asmBackward = q.env.asmMode != 1;
            const bool narrow = ((q.flags & CPECAN_FLAG_ASM_NARROW_BANDS) || q.env.asmNarrow) && d.asmBackward;
            const int cells = d.build->rows == ASM_L && q.maxWidth <= ASM_MAX_WIDTH ? ASM_L
                              : d.build->rows == ASM2_L && q.maxWidth <= ASM2_MAX_WIDTH && narrow ? ASM2_L : 0;
            d.asmSweeps = d.asmPlan && q.env.asmMode != 0 && d.build->post_asm && cells != 0;
            d.asmCells = d.asmSweeps ? cells : 0;
            /* the fused build in the place of the ring build of as many rows, where the batch asks for it */
            if (q.mode == CPECAN_MODE_EXPECTATIONS)
                for (const FusedStandIn &f : FUSED_STAND_INS)
                    if (d.build == f.ring && ((d.flags & f.flag) || (f.env && q.env.*f.env))) d.build = f.fused;
            /* the strawMan machine's E-step on the wave kernels sums its expectations inside the sweep back (same box,
             * configs[3] on one context: 97.2 against 150.8 ms per iteration); CPECAN_EXPECT_FUSED=0 keeps
             * the ring of backward cells and the expectation kernel.  A fused build of the workgroup family, or of the
             * vanilla machine, has no other form of the E-step. */
            d.fused = q.mode == CPECAN_MODE_EXPECTATIONS && d.build->backward_fx && (!d.build->expect || !q.env.ringEstep);
            d.expectResweep = d.fused ? q.env.expectResweep : 0;
        }
    }
    d.wave5 = q.machine == DNA5 && !debug && !unbanded && q.maxWidth <= CP_WAVE5_MAX_WIDTH && !q.env.wave5Off &&
              !(q.flags & CPECAN_FLAG_GENERAL_KERNEL);
    /* the 4-state machine's wave kernels are opt-in, by the flag alone (no environment variable), posterior decode on
     * banded matrices; a wider band runs on the general kernel, as every 4-state batch without the flag does */
    d.wave4 = q.machine == SM4 && q.mode == CPECAN_MODE_POSTERIOR && (q.flags & CPECAN_FLAG_SM4_WAVE) && !debug && !unbanded &&
              q.maxWidth <= CP_WAVE4_MAX_WIDTH && !(q.flags & CPECAN_FLAG_GENERAL_KERNEL);
    return d;
}

/* The plan of one alignment for the assembly sweeps: its traceback windows (getPosteriorProbsWithBanding's schedule,
 * impl/pairwiseAligner.c:917-921 -- a function of the band alone; the same walk as the window count in batch_create) and,
 * per diagonal, whether the band's edges step and whether the forward sweep keeps all three states of the diagonal
 * (forward_window() of cpecan_kernel_wave.hip works the same rule out on the device).  tab: (first, last) column per
 * diagonal.  belowToo: the compiled sweep back reads what the forward sweep leaves (CPECAN_ASM=1: Dispatch::asmBackward
 * is false).  Runs on the worker threads of build_bands: it reads no environment. */
static void build_asm_plan(const int *tab, long long nDiag, const cpecan_band_params &bp, bool belowToo,
                           std::vector<AsmPlanWin> &wins, AsmPlanCtl *ctl) {
    const long long D = nDiag - 1;
    memset(ctl, 0, (size_t) (D / ASM_BLOCK + 2) * sizeof(AsmPlanCtl));
    wins.clear();
    long long tracedBackTo = 0, cells = 1;
    int d0 = 0;
    for (long long k = 1; k <= D; k++) {
        const int xmn = tab[2 * k], xmx = tab[2 * k + 1];
        if (xmn != tab[2 * k - 2]) ctl[k >> 6].stepMin |= 1ull << (k & 63);
        if (xmx != tab[2 * k - 1]) ctl[k >> 6].stepMax |= 1ull << (k & 63);
        cells += xmx - xmn + 1;
        const bool atEnd = k == D;
        const bool tb = k >= tracedBackTo + bp.minDiagsBetweenTraceBack && xmx - xmn + 1 <= bp.diagonalExpansion * 2 + 1;
        if (!(atEnd || tb)) continue;
        AsmPlanWin w{};
        w.d0 = d0;
        w.top = (int) k;
        w.from = (int) (k - (atEnd ? 0 : bp.traceBackDiagonals + 1));
        w.to = (int) tracedBackTo;
        w.atEnd = atEnd ? 1 : 0;
        w.xminTop = xmn;
        w.xmaxTop = xmx;
        w.cells = cells;
        w.xmin0 = tab[2 * d0];
        w.xmax0 = tab[2 * d0 + 1];
        w.tpost0 = std::min(w.top, w.from);
        wins.push_back(w);
        d0 = (int) k;
        tracedBackTo = w.from;
    }
    for (size_t wi = 0; wi < wins.size(); wi++) {
        AsmPlanWin &w = wins[wi];
        w.nWindows = (int) wins.size();
        /* all three states: the two diagonals a launch resumes from and every diagonal with a totalProbability refresh of
         * the window that decodes it (every 10th decoded diagonal, counted down from the window's first); the compiled
         * sweep back (CPECAN_ASM=1: tests, timing) also reads the diagonal below a refresh, the assembly one does not
         * (gen_sweeps.py: the refresh's second half is F.match + B.match of the diagonal above); everything where windows
         * are shorter than the traceback margin */
        const bool endW = w.atEnd != 0;
        const int tpA = w.tpost0;
        int tpB = tpA;
        bool allFull = false;
        if (!endW) {
            tpB = wins[wi + 1].tpost0;
            allFull = tpB < w.top;
        }
        for (int dj = w.d0 + 1; dj <= w.top; dj++) {
            const int rA = ((tpA - dj) % 10 + 10) % 10, rB = endW ? 99 : ((tpB - dj) % 10 + 10) % 10;
            const int rHere = dj <= w.from ? rA : rB, rAbove = dj + 1 <= w.from ? rA : rB;
            if (allFull || dj >= w.top - 1 || rHere == 0 || (belowToo && rAbove == 1)) ctl[dj >> 6].full |= 1ull << (dj & 63);
        }
    }
}

extern "C" {

const char *cpecan_hip_last_error(void) { return g_err.c_str(); }
const char *cpecan_hip_version(void) { return "cpecan-signal_amd 0.1 (gfx950)"; }

int cpecan_hip_device_count(int *count) {
    if (!count) return fail(CPECAN_EINVAL, "count is NULL");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) {
        *count = 0;
        return fail(CPECAN_ENODEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e));
    }
    *count = n;
    return CPECAN_OK;
}

} // extern "C"

/* Every run of the context's batches is over, on whatever lanes it went (a lane also carries the runs of other
 * contexts' batches, so no lane is waited for): what guards the model tables those runs read.  The context's prep
 * stream is made to wait for the runs' end events under the list's lock (which only queues the waits), and the host
 * waits for the prep stream after it: other threads' contexts are not held up for the length of a pass. */
static std::mutex g_batchesMu; /* the contexts' batch lists */

hipError_t ctx_fence(cpecan_ctx *c) {
    hipError_t r = hipSuccess;
    {
        std::lock_guard<std::mutex> g(g_batchesMu);
        for (cpecan_batch *b : c->batches)
            if (b->ran) {
                hipError_t e = hipStreamWaitEvent(c->prep, b->ev2, 0);
                if (e != hipSuccess) e = hipEventSynchronize(b->ev2); /* (the wait could not be queued: wait here) */
                if (r == hipSuccess) r = e;
            }
    }
    const hipError_t e = hipStreamSynchronize(c->prep);
    return r != hipSuccess ? r : e;
}

int pinned_slots(cpecan_ctx *c, size_t want) {
    if (c->pinnedBytes >= want) return CPECAN_OK;
    if (c->pinned) (void) hipHostFree(c->pinned);
    c->pinned = nullptr;
    c->pinnedBytes = 0;
    HIP_TRY(hipHostMalloc(&c->pinned, want, hipHostMallocDefault));
    c->pinnedBytes = want;
    return CPECAN_OK;
}

extern "C" {

int cpecan_hip_ctx_create(int device, cpecan_ctx **out) {
    if (!out) return fail(CPECAN_EINVAL, "ctx is NULL");
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(CPECAN_ENODEVICE, "no HIP device is available; this library has no CPU path");
    if (device < 0 || device >= n) return fail(CPECAN_EINVAL, "device %d out of range (%d)", device, n);
    HIP_TRY(hipSetDevice(device));
    cpecan_ctx *c = new (std::nothrow) cpecan_ctx();
    if (!c) return fail(CPECAN_EINVAL, "out of host memory");
    c->device = device;
    /* the lanes first: a process gets few hardware queues (four by default) and the first streams made have one each */
    hipError_t e = lanes_create(device, &c->lanes);
    if (e != hipSuccess) {
        delete c;
        return fail(CPECAN_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
    }
    c->stream = c->lanes->fwd;
    int least = 0, greatest = 0;
    (void) hipDeviceGetStreamPriorityRange(&least, &greatest);
    e = hipStreamCreateWithPriority(&c->prep, hipStreamNonBlocking, greatest);
    if (e != hipSuccess) {
        lanes_release(c->lanes);
        delete c;
        return fail(CPECAN_EHIP, "hipStreamCreateWithPriority: %s", hipGetErrorString(e));
    }
    *out = c;
    return CPECAN_OK;
}

int cpecan_hip_ctx_destroy(cpecan_ctx *c) {
    if (!c) return CPECAN_OK;
    (void) hipSetDevice(c->device);
    /* the model tables go back to the allocator's cache below: no run of this context's batches may still read them,
     * whichever lanes it went on.  The lanes themselves live on while a batch of another context holds them. */
    (void) ctx_fence(c);
    if (c->prep) (void) hipStreamSynchronize(c->prep);
    {
        std::lock_guard<std::mutex> g(g_batchesMu);
        for (cpecan_batch *b : c->batches) b->ctx = nullptr; /* (a batch may be destroyed after its context) */
        c->batches.clear();
    }
    lanes_release(c->lanes);
    c->lanes = nullptr;
    c->stream = nullptr;
    if (c->prep) (void) hipStreamDestroy(c->prep);
    if (c->pinned) (void) hipHostFree(c->pinned);
    for (auto *t : c->hdpTables) delete t;
    c->hdpTables.clear();
    delete c;
    (void) hipGetLastError();
    return CPECAN_OK;
}

int cpecan_hip_trim_cache(void) {
    dev_cache().trim(0);
    pinned_cache().trim(0);
    (void) hipGetLastError();
    return CPECAN_OK;
}

int cpecan_hip_cache_capacity(cpecan_ctx *c, int64_t *deviceBytes) {
    if (!c || !deviceBytes) return fail(CPECAN_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(c->device)); /* (the default is worked out from the card's memory) */
    DevCache &cache = dev_cache();
    std::lock_guard<std::mutex> g(cache.lock);
    *deviceBytes = (int64_t) cache.cap();
    return CPECAN_OK;
}

int cpecan_hip_ctx_memory(cpecan_ctx *c, int64_t *live, int64_t *peak, int32_t resetPeak) {
    if (!c) return fail(CPECAN_EINVAL, "ctx is NULL");
    if (live) *live = c->mem->live;
    if (peak) *peak = c->mem->peak;
    if (resetPeak) c->mem->peak = c->mem->live;
    return CPECAN_OK;
}

int cpecan_hip_ctx_set_memory_limit(cpecan_ctx *c, int64_t bytes) {
    if (!c || bytes < 0) return fail(CPECAN_EINVAL, "bad argument");
    c->mem->limit = bytes;
    return CPECAN_OK;
}

int cpecan_hip_batch_device_bytes(cpecan_batch *b, int64_t *bytes) {
    if (!b || !bytes) return fail(CPECAN_EINVAL, "bad argument");
    *bytes = b->mem->live;
    return CPECAN_OK;
}

int cpecan_hip_ctx_stream(cpecan_ctx *c, void **stream) {
    if (!c || !stream) return fail(CPECAN_EINVAL, "NULL argument");
    *stream = (void *) c->stream;
    return CPECAN_OK;
}

int cpecan_hip_selftest_division(cpecan_ctx *c, int64_t n, uint64_t seed, int64_t *mismatches) {
    if (!c || n <= 0 || !mismatches) return fail(CPECAN_EINVAL, "bad argument");
    HIP_TRY(hipSetDevice(c->device));
    DevBuf<unsigned long long> bad;
    StreamFence fence{ c->prep, nullptr };
    HIP_TRY(bad.alloc(1));
    HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(unsigned long long), c->prep));
    if (cpecan_systolic_divtest(c->prep, n, seed, bad.p) != 0)
        return fail(CPECAN_EHIP, "division self-test launch failed");
    unsigned long long h = 0;
    HIP_TRY(hipStreamSynchronize(c->prep));
    HIP_TRY(hipMemcpy(&h, bad.p, sizeof h, hipMemcpyDeviceToHost));
    *mismatches = (int64_t) h;
    return CPECAN_OK;
}

/* emissions_signal_getDurationProb -> poissonPosteriorProb (impl/stateMachine.c:345-370, :551-554): the log
 * posterior of n k-mers given the event's duration (its third value), with the host libm's log */
static double echelon_duration(const double *event, int n) {
    static const double logFactorial[6] = { 0.0, 0.0, 0.69314718056, 1.79175946923, 3.17805383035, 4.78749174278 };
    const double lambda = event[2] / 0.00332005312085;
    return (n + 1) * 0.1397619423751586 + n * log(lambda) - logFactorial[n] - 2 * lambda;
}

int cpecan_hip_batch_destroy(cpecan_batch *b) {
    if (!b) return CPECAN_OK;
    /* the batch keeps its own device id: a caller (a garbage collector, say) may destroy the context first, and
     * nothing here may depend on it then */
    (void) hipSetDevice(b->device);
    Lap lap("batch_destroy");
    /* the batch's device memory goes back to the allocator's cache, not to the driver (which would wait for the
     * device): nothing of this batch may still be running when another batch is handed the blocks */
    if (b->ev2 && b->ran) (void) hipEventSynchronize(b->ev2);
    if (b->ev0) (void) hipEventDestroy(b->ev0);
    if (b->ev1) (void) hipEventDestroy(b->ev1);
    if (b->ev2) (void) hipEventDestroy(b->ev2);
    for (hipEvent_t e : b->evStage) (void) hipEventDestroy(e);
    for (hipEvent_t e : b->evJoin) (void) hipEventDestroy(e);
    if (b->evFork) (void) hipEventDestroy(b->evFork);
    if (b->gStreamOwned)
        for (hipStream_t st : b->gStream) (void) hipStreamDestroy(st);
    for (hipStream_t st : b->gStreamB) (void) hipStreamDestroy(st);
    lanes_release(b->runLanes);
    {
        std::lock_guard<std::mutex> g(g_batchesMu);
        if (b->ctx) b->ctx->batches.erase(std::remove(b->ctx->batches.begin(), b->ctx->batches.end(), b), b->ctx->batches.end());
    }
    for (hipEvent_t e : b->evPost) (void) hipEventDestroy(e);
    release_readback(b);
    delete b;
    (void) hipGetLastError(); /* a failed clean-up call must not surface as the "last error" of a later launch */
    return CPECAN_OK;
}

#define B_TRY(expr)                                                                          \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess) {                                                              \
            int rc_ = fail(CPECAN_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), \
                           __FILE__, __LINE__);                                              \
            cpecan_hip_batch_destroy(b);                                                     \
            return rc_;                                                                      \
        }                                                                                    \
    } while (0)

} // extern "C"

/* what a create call was given (events, or for DNA against DNA yChars: nEvents then counts its bases) */
struct BatchInput {
    const cpecan_item *items;
    int64_t nItems;
    const char *xChars;
    int64_t nX;
    const double *events;
    const char *yChars;
    int64_t nEvents;
    const int64_t *anchors;
    int64_t nAnchorPairs;
    const cpecan_band_params *params;
    int mode;
    bool unbanded;
};

/* The host's plan of a batch's bands (integer work): the band of every item as matrix columns (first, last) per diagonal
 * -- what the register-resident kernels read -- written straight into a pinned block; the x-y intervals and the cell
 * prefix sums of the general kernel only when the batch will (or, on a second build, turns out to) run on it; the
 * traceback schedule; where every item's share of each buffer begins. */
struct BandPlan {
    std::vector<DevItem> items;
    PinnedBuf<int> tab;
    std::vector<int, NoInit<int>> L, R; /* (general) */
    std::vector<long long, NoInit<long long>> pre;
    bool general = false; /* L, R and pre are built */
    long long diagTotal = 0, maxDiags = 0;
    int maxWidth = 0, maxSpan = 1, maxWindows = 0, maxLX = 0;
    long long maxLXY = 0;        /* the longest sequence of the batch, either side */
    bool edgesStepByOne = true; /* band edges move by at most one k-mer per diagonal */
    long long cellTotal = 0, pairTotal = 0, totTotal = 0, bwsTotal = 0, trackTotal = 0;
    std::vector<long long> trackBase;
    /* the assembly sweeps' plan (build_asm_plan), for the batches that can run on them */
    bool wantAsm = false, asmBelowToo = false;
    std::vector<std::vector<AsmPlanWin>> asmWins;
    std::vector<long long> asmOff;
    PinnedBuf<AsmPlanCtl> asmCtl;
    long long asmCtlTotal = 0;
};

/* per-item bounds and model ids; the items as the device reads them, offsets in one serial pass */
static int check_items(const cpecan_ctx *c, Machine machine, const BatchInput &in, BandPlan &plan) {
    const MachineRow &m = MACHINES[machine];
    const int kmerTail = m.x == X_CHARS ? 0 : 5; /* the characters of the last k-mer past lX */
    const int nModels = c->tables[machine].n;
    plan.items.resize((size_t) in.nItems);
    for (int64_t i = 0; i < in.nItems; i++) {
        const cpecan_item &s = in.items[i];
        if (s.lX < 0 || s.lY < 0 || s.x_offset < 0 || s.y_offset < 0 || s.n_anchors < 0 ||
            s.anchor_offset < 0 || s.x_offset + s.lX + (s.lX > 0 ? kmerTail : 0) > in.nX ||
            s.y_offset + s.lY > in.nEvents || s.anchor_offset + s.n_anchors > in.nAnchorPairs)
            return fail(CPECAN_EINVAL, "item %lld points outside the supplied buffers", (long long) i);
        if (machine == ECHELON && (s.reserved < 0 || s.reserved > 30 || (s.lX > 0 && s.x_offset + s.lX + 5 + s.reserved > in.nX)))
            return fail(CPECAN_EINVAL, "item %lld: its look-ahead (reserved = %d) points outside the supplied characters",
                        (long long) i, s.reserved);
        if (s.model_id < 0 || s.model_id >= nModels)
            return fail(CPECAN_EINVAL, "item %lld: unknown model id %d", (long long) i, s.model_id);
        if (s.lX + s.lY >= (1ll << 30)) return fail(CPECAN_EINVAL, "item %lld too long", (long long) i);
        DevItem &d = plan.items[(size_t) i];
        d.lX = s.lX; d.lY = s.lY; d.xOff = s.x_offset; d.yOff = s.y_offset;
        d.anchorOff = s.anchor_offset; d.nAnchors = s.n_anchors;
        d.model = s.model_id; d.raggedL = s.ragged_left ? 1 : 0; d.raggedR = s.ragged_right ? 1 : 0;
        d.diagBase = plan.diagTotal;
        plan.diagTotal += s.lX + s.lY + 1;
        plan.maxDiags = std::max<long long>(plan.maxDiags, s.lX + s.lY + 1);
    }
    return CPECAN_OK;
}

/* Whether an item of a vanilla batch meets a k-mer that is none (cpecan_item_meets_no_kmer, cpecan_band_extent.h) */
static bool vanilla_meets_no_kmer(const BatchInput &in) {
    for (int64_t i = 0; i < in.nItems; i++)
        if (cpecan_item_meets_no_kmer(in.xChars + in.items[i].x_offset, in.items[i].lX)) return true;
    return false;
}

/* The bands themselves, the items dealt to the host threads (band, cell prefix, traceback schedule: ~15 000 diagonals
 * per C3 read).  A thread's working copy of one item's intervals stays in its cache. */
static int build_bands(const BatchInput &in, BandPlan &plan, bool general) {
    struct ItemStats {
        int maxSpan = 1, windows = 0, badItem = -1, badRc = 0;
        bool edgesStepByOne = true;
    };
    const cpecan_band_params &bp = *in.params;
    const long long maxDiags = plan.maxDiags;
    if (general) {
        plan.L.resize((size_t) plan.diagTotal);
        plan.R.resize((size_t) plan.diagTotal);
        plan.pre.resize((size_t) plan.diagTotal);
        plan.general = true;
    }
    const int nt = (int) std::min<int64_t>(plan.diagTotal > 2000000 ? host_threads() : 1, in.nItems);
    std::vector<ItemStats> stats((size_t) nt);
    auto work = [&](int w) {
        ItemStats &st = stats[(size_t) w];
        std::vector<int, NoInit<int>> own(general ? 0 : 2 * (size_t) maxDiags);
        for (int64_t i = w; i < in.nItems; i += nt) {
            const cpecan_item &s = in.items[i];
            DevItem &d = plan.items[(size_t) i];
            const long long nDiag = s.lX + s.lY + 1;
            int *Lp = general ? plan.L.data() + d.diagBase : own.data();
            int *Rp = general ? plan.R.data() + d.diagBase : own.data() + maxDiags;
            /* getAlignedPairsWithoutBanding builds its band from no anchors, expansion 2 (:1532) */
            int rc = cpecan_band_construct(in.unbanded || !in.anchors ? nullptr : in.anchors + 2 * s.anchor_offset,
                                           in.unbanded ? 0 : s.n_anchors, s.lX, s.lY,
                                           in.unbanded ? 2 : bp.diagonalExpansion, Lp, Rp);
            if (rc != CPECAN_OK) {
                if (st.badItem < 0) { st.badItem = (int) i; st.badRc = rc; }
                continue;
            }
            long long cells = 0;
            int maxW = 0;
            long long *pre = general ? plan.pre.data() + d.diagBase : nullptr;
            int *tab = plan.tab.p + d.diagBase * 2;
            /* traceback schedule of getPosteriorProbsWithBanding (:917-918): longest span of forward
             * diagonals that must be resident at once, and the edge-step property the register-resident
             * kernels rely on */
            long long tracedBackTo = 0;
            int windows = 0, stepByOne = 1, prev[2] = { 0, 0 }, col[2];
            for (long long k = 0; k < nDiag; k++) {
                if (pre) pre[k] = cells;
                const int wd = cpecan_diag_extent(k, Lp[k], Rp[k], prev, col, &stepByOne);
                cells += wd;
                maxW = std::max(maxW, wd);
                tab[k * 2] = col[0];
                tab[k * 2 + 1] = col[1];
                if (k >= 1) {
                    const bool atEnd = k == nDiag - 1;
                    const bool tb = k >= tracedBackTo + bp.minDiagsBetweenTraceBack && wd <= bp.diagonalExpansion * 2 + 1;
                    if (atEnd || tb) {
                        windows++;
                        st.maxSpan = (int) std::max<long long>(st.maxSpan, k - tracedBackTo + 1);
                        tracedBackTo = k - (bp.traceBackDiagonals + 1);
                    }
                }
                prev[0] = col[0];
                prev[1] = col[1];
            }
            if (!stepByOne) st.edgesStepByOne = false;
            d.nCells = cells;
            d.maxWidth = maxW;
            st.windows = std::max(st.windows, windows);
            if (plan.wantAsm)
                build_asm_plan(tab, nDiag, bp, plan.asmBelowToo, plan.asmWins[(size_t) i], plan.asmCtl.p + plan.asmOff[(size_t) i]);
        }
    };
    if (nt <= 1) work(0);
    else {
        std::vector<std::thread> pool;
        for (int w = 0; w < nt; w++) pool.emplace_back(work, w);
        for (auto &t : pool) t.join();
    }
    plan.maxSpan = 1;
    plan.maxWindows = 0;
    plan.edgesStepByOne = true;
    int bad = -1, badRc = 0;
    for (const ItemStats &st : stats) {
        plan.maxSpan = std::max(plan.maxSpan, st.maxSpan);
        plan.maxWindows = std::max(plan.maxWindows, st.windows);
        plan.edgesStepByOne = plan.edgesStepByOne && st.edgesStepByOne;
        if (st.badItem >= 0 && (bad < 0 || st.badItem < bad)) { bad = st.badItem; badRc = st.badRc; }
    }
    if (bad >= 0) return fail(badRc, "item %lld: anchors do not describe a valid band", (long long) bad);
    return CPECAN_OK;
}

/* the bands, then every item's share of the batch's buffers (early: the kernel choice before the bands are known) */
static int plan_bands(const BatchInput &in, const MachineRow &m, const Dispatch &early, BandPlan &plan) {
    const bool general = early.kernel == CPECAN_KERNEL_GENERAL;
    plan.wantAsm = early.asmPlan;
    plan.asmBelowToo = !early.asmBackward;
    if (plan.wantAsm) {
        plan.asmWins.resize((size_t) in.nItems);
        plan.asmOff.resize((size_t) in.nItems);
        for (int64_t i = 0; i < in.nItems; i++) {
            plan.asmOff[(size_t) i] = plan.asmCtlTotal;
            plan.asmCtlTotal += (in.items[i].lX + in.items[i].lY) / ASM_BLOCK + 2;
        }
        HIP_TRY(plan.asmCtl.alloc((size_t) plan.asmCtlTotal));
    }
    HIP_TRY(plan.tab.alloc((size_t) plan.diagTotal * 2 + 2));
    const int rc = build_bands(in, plan, general);
    if (rc != CPECAN_OK) return rc;
    plan.trackBase.resize((size_t) in.nItems);
    for (int64_t i = 0; i < in.nItems; i++) {
        const cpecan_item &s = in.items[i];
        DevItem &d = plan.items[(size_t) i];
        const long long nDiag = s.lX + s.lY + 1;
        plan.trackBase[(size_t) i] = plan.trackTotal;
        plan.trackTotal += s.lX + 1;
        plan.maxLX = std::max<int>(plan.maxLX, (int) s.lX);
        plan.maxLXY = std::max<long long>(plan.maxLXY, std::max<long long>(s.lX, s.lY));
        plan.maxWidth = std::max(plan.maxWidth, d.maxWidth);
        d.cellBase = plan.cellTotal;
        plan.cellTotal += d.nCells;
        d.pairBase = plan.pairTotal;
        d.pairCap = m.pairCapFactor * (s.lX + s.lY) + 64;
        plan.pairTotal += d.pairCap;
        d.totBase = plan.totTotal;
        d.totCap = (nDiag + 9) / 10 + nDiag / std::max<long long>(1, in.params->minDiagsBetweenTraceBack -
                                                                     in.params->traceBackDiagonals - 1) + 4;
        plan.totTotal += d.totCap;
        d.bwsBase = plan.bwsTotal;
        plan.bwsTotal += 3ll * d.maxWidth * m.states;
    }
    return CPECAN_OK;
}

/* the batch object, registered with its context; no device work yet */
static cpecan_batch *new_batch(cpecan_ctx *c, Machine machine, const BatchInput &in, const BandPlan &plan, const Dispatch &d) {
    const MachineRow &m = MACHINES[machine];
    const cpecan_band_params &bp = *in.params;
    cpecan_batch *b = new (std::nothrow) cpecan_batch();
    if (!b) return nullptr;
    b->ctx = c;
    b->mem = std::make_shared<MemAccount>();
    b->mem->of = c->mem;
    {
        std::lock_guard<std::mutex> g(g_batchesMu);
        c->batches.push_back(b);
    }
    b->device = c->device;
    b->modelEpoch = c->modelEpoch;
    b->nItems = in.nItems;
    b->mode = in.mode;
    b->flags = d.flags;
    b->machine = machine;
    b->kernel = d.kernel;
    b->wave5 = d.wave5;
    b->wave4 = d.wave4;
    b->maxWidth = plan.maxWidth;
    b->compactPairs = plan.maxLXY + m.xReach < 65536;
    b->nModels = c->tables[machine].n;
    b->expectLen = m.expectLen;
    b->P.threshold = bp.threshold;
    b->P.minDiags = bp.minDiagsBetweenTraceBack;
    b->P.tbDiags = bp.traceBackDiagonals;
    b->P.expansion = bp.diagonalExpansion;
    b->P.mode = in.mode;
    b->P.debug = (d.flags & CPECAN_FLAG_DEBUG_DUMP) ? 1 : 0;
    b->P.unbanded = in.unbanded ? 1 : 0;
    b->P.scanDecode = (d.flags & CPECAN_FLAG_SCAN_DECODE) ? 1 : 0;
    b->P.logThrSlack = bp.threshold > 0.0 ? log(bp.threshold) - 1e-3 : -INFINITY;
    b->P.ldsWidth = 0; /* (set per launch by the kernels that use it) */
    /* what the kernel choice came to is the batch's: nothing after it changes the build or the form of the E-step */
    b->sy = d.build ? d.build : SY_BUILDS[3];
    b->fused = d.fused;
    b->P.expectResweep = d.expectResweep;
    if (d.build) b->trackRow = b->sy->once->trackRowDoubles;
    b->hItems = plan.items;
    return b;
}

/* From here on the batch exists: a step that fails has destroyed it (B_TRY) before it returns its code. */

static int upload_sequences(cpecan_batch *b, const BatchInput &in) {
    cpecan_ctx *c = b->ctx;
    const MachineRow &m = MACHINES[b->machine];
    const int64_t nItems = in.nItems, nX = in.nX, nEvents = in.nEvents;
    B_TRY(b->items.alloc((size_t) nItems));
    B_TRY(hipMemcpyAsync(b->items.p, b->hItems.data(), (size_t) nItems * sizeof(DevItem), hipMemcpyHostToDevice, c->prep));
    B_TRY(b->chars.alloc((size_t) nX + 8));
    B_TRY(hipMemsetAsync(b->chars.p, 0, (size_t) nX + 8, c->prep));
    B_TRY(hipMemcpyAsync(b->chars.p, in.xChars, (size_t) nX, hipMemcpyHostToDevice, c->prep));
    B_TRY(b->kidx.alloc((size_t) nX + 8));
    if (in.yChars) {
        B_TRY(b->charsY.alloc((size_t) nEvents + 8));
        B_TRY(hipMemsetAsync(b->charsY.p, 0, (size_t) nEvents + 8, c->prep));
        B_TRY(hipMemcpyAsync(b->charsY.p, in.yChars, (size_t) nEvents, hipMemcpyHostToDevice, c->prep));
    } else if (m.yAux) {
        /* emissions_signal_logInvGaussPdf takes log(eventNoise) per cell (host libm, :325): an array of its own for the
         * general kernel, and in the batch's own copy of the events in place of the duration, which nothing on the
         * device reads (the wave kernels stage events from this one array) */
        std::vector<double, NoInit<double>> ev3((size_t) 3 * nEvents), ln((size_t) nEvents + 1);
        for (int64_t i = 0; i < nEvents; i++) {
            ln[(size_t) i] = log(in.events[3 * i + 1]);
            ev3[(size_t) 3 * i] = in.events[3 * i];
            ev3[(size_t) 3 * i + 1] = in.events[3 * i + 1];
            ev3[(size_t) 3 * i + 2] = ln[(size_t) i];
        }
        B_TRY(b->events.alloc((size_t) 3 * nEvents + 8));
        B_TRY(b->logNoise.alloc((size_t) nEvents + 8));
        B_TRY(hipMemcpyAsync(b->events.p, ev3.data(), (size_t) 3 * nEvents * sizeof(double), hipMemcpyHostToDevice, c->prep));
        B_TRY(hipMemcpyAsync(b->logNoise.p, ln.data(), (size_t) nEvents * sizeof(double), hipMemcpyHostToDevice, c->prep));
        B_TRY(hipStreamSynchronize(c->prep)); /* ev3 and ln end here */
    } else {
        B_TRY(b->events.alloc((size_t) 3 * nEvents + 8));
        B_TRY(hipMemcpyAsync(b->events.p, in.events, (size_t) 3 * nEvents * sizeof(double), hipMemcpyHostToDevice, c->prep));
    }
    if (b->machine == ECHELON) { /* emissions_signal_getDurationProb (:551-554) of 0..5 k-mers per event */
        std::vector<double> du((size_t) 6 * nEvents + 6);
        for (int64_t i = 0; i < nEvents; i++)
            for (int k = 0; k < 6; k++) du[(size_t) (6 * i + k)] = echelon_duration(in.events + 3 * i, k);
        B_TRY(b->duration.alloc((size_t) 6 * nEvents + 8));
        B_TRY(hipMemcpyAsync(b->duration.p, du.data(), (size_t) 6 * nEvents * sizeof(double), hipMemcpyHostToDevice, c->prep));
        std::vector<long long> xe((size_t) nItems);
        for (int64_t i = 0; i < nItems; i++) xe[(size_t) i] = in.items[i].lX > 0 ? in.items[i].lX + 5 + in.items[i].reserved : 0;
        B_TRY(b->xEnd.alloc((size_t) nItems));
        B_TRY(hipMemcpyAsync(b->xEnd.p, xe.data(), (size_t) nItems * sizeof(long long), hipMemcpyHostToDevice, c->prep));
        B_TRY(hipStreamSynchronize(c->prep)); /* du and xe end here */
    }
    B_TRY(hipStreamSynchronize(c->prep));
    return CPECAN_OK;
}

/* (the anchors stay on the host: the bands they describe were built there) */
static int alloc_outputs(cpecan_batch *b, const BandPlan &plan) {
    cpecan_ctx *c = b->ctx;
    const size_t nItems = (size_t) b->nItems;
    B_TRY(b->pairs.alloc((size_t) plan.pairTotal * 3));
    B_TRY(b->pairLogp.alloc((size_t) plan.pairTotal));
    B_TRY(b->nPairs.alloc(nItems));
    B_TRY(b->nTot.alloc(nItems));
    B_TRY(b->nCells.alloc(nItems));
    B_TRY(b->totXay.alloc((size_t) plan.totTotal));
    B_TRY(b->totVal.alloc((size_t) plan.totTotal));
    B_TRY(b->expect.alloc((size_t) std::max(b->nModels, 1) * b->expectLen));
    B_TRY(hipMemsetAsync(b->expect.p, 0, b->expect.n * sizeof(double), c->prep));
    b->hNCells.resize(nItems);
    for (size_t i = 0; i < nItems; i++) b->hNCells[i] = b->hItems[i].nCells;
    B_TRY(hipStreamSynchronize(c->prep));
    return CPECAN_OK;
}

/* the general kernel: the bands as x-y intervals with their cell prefix sums, every forward cell, a backward workspace */
static int general_storage(cpecan_batch *b, const BatchInput &in, BandPlan &plan) {
    cpecan_ctx *c = b->ctx;
    if (!plan.general) { /* the band turned out too wide (or too ragged) for the register-resident kernels */
        const int rc = build_bands(in, plan, true);
        if (rc != CPECAN_OK) {
            cpecan_hip_batch_destroy(b);
            return rc;
        }
    }
    B_TRY(b->bandL.alloc(plan.L.size()));
    B_TRY(b->bandR.alloc(plan.R.size()));
    B_TRY(b->cellPrefix.alloc(plan.pre.size()));
    B_TRY(hipMemcpyAsync(b->bandL.p, plan.L.data(), plan.L.size() * sizeof(int), hipMemcpyHostToDevice, c->prep));
    B_TRY(hipMemcpyAsync(b->bandR.p, plan.R.data(), plan.R.size() * sizeof(int), hipMemcpyHostToDevice, c->prep));
    B_TRY(hipMemcpyAsync(b->cellPrefix.p, plan.pre.data(), plan.pre.size() * sizeof(long long), hipMemcpyHostToDevice, c->prep));
    B_TRY(b->Fstore.alloc((size_t) plan.cellTotal * MACHINES[b->machine].states));
    B_TRY(b->Bstore.alloc((size_t) plan.bwsTotal));
    if (b->P.debug) {
        B_TRY(b->dbgB.alloc((size_t) plan.cellTotal * 3));
        B_TRY(hipMemsetAsync(b->dbgB.p, 0xff, (size_t) plan.cellTotal * 3 * sizeof(double), c->prep));
    }
    return CPECAN_OK;
}

/* the register-resident kernels: one workgroup per alignment and launch; the ring of forward diagonals lives per
 * alignment because the forward and backward kernels of a window are separate launches */
static int sweep_storage(cpecan_batch *b, const BandPlan &plan, const Dispatch &d, const BatchEnv &env, Lap &lap) {
    cpecan_ctx *c = b->ctx;
    const int64_t nItems = b->nItems;
    const int maxWindows = plan.maxWindows, maxSpan = plan.maxSpan;
    b->nWorkers = (int) nItems;
    b->nWindows = maxWindows;
    b->ringD = 64;
    /* the kernels mask with ringD-1.  The wave kernels sweep window w back while the forward sweep of window w+1
     * is writing: the ring holds two windows -- three where the assembly sweeps may run (set up in asm_setup; the same
     * conditions but for what is not known yet): there the forward sweep of window w+2 does not wait for the totals
     * and the decode of window w, whose re-sweep kernel may still read that window's rows */
    const int ringWindows = !b->sy->wave || maxWindows <= 1 ? 1
                            : d.asmSweeps && maxWindows > 2 && !(b->flags & CPECAN_FLAG_SMALL_FOOTPRINT) ? 3 : 2;
    while (b->ringD < (ringWindows > 1 ? ringWindows * maxSpan + 8 : maxSpan + 4)) b->ringD *= 2;
    /* the wave kernels keep one more row behind the ring: the -inf row lanes without a cell read */
    b->ringDoubles = (long long) (b->ringD + (b->sy->wave ? 1 : 0)) * b->sy->ringRowDoubles;
    b->ringDoubles += env.ringPad;
    b->maxLX = plan.maxLX;
    B_TRY(b->Fstore.alloc((size_t) nItems * (size_t) b->ringDoubles));
    lap("ring allocation");
    /* the band as matrix columns per diagonal */
    B_TRY(b->bandTab.alloc((size_t) plan.diagTotal * 2 + 2));
    B_TRY(hipMemcpyAsync(b->bandTab.p, plan.tab.p, (size_t) plan.diagTotal * 2 * sizeof(int), hipMemcpyHostToDevice, c->prep));
    {
        int G = env.systolicGroups ? env.systolicGroups : b->sy->wave ? 1 : 2;
        if ((int64_t) G > nItems) G = (int) nItems;
        b->nGroups = G;
        b->gStream.assign((size_t) G, nullptr);
        b->evJoin.assign((size_t) G, nullptr);
        /* a wave batch of one group runs on lane sets (cpecan_run.hip): no streams of its own, so that a chain of
         * batches stays within the four hardware queues a process gets */
        b->gStreamOwned = !(b->sy->wave && G == 1);
        if (b->gStreamOwned)
            for (auto &st : b->gStream) B_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        else {
            b->gStream.clear();
            B_TRY(lanes_sweeps(c->lanes));
        }
        if (b->sy->wave && b->gStreamOwned) {
            b->gStreamB.assign((size_t) G, nullptr);
            for (auto &st : b->gStreamB) B_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
        }
        for (auto &e : b->evJoin) B_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        B_TRY(hipEventCreateWithFlags(&b->evFork, hipEventDisableTiming));
    }
    B_TRY(hipStreamSynchronize(c->prep));
    lap("band table upload, streams");
    if (b->mode == CPECAN_MODE_EXPECTATIONS && !b->fused)
        B_TRY(b->Bring.alloc((size_t) nItems * (size_t) b->ringD * (size_t) b->sy->bringRowDoubles));
    b->stateBytes = b->sy->once->stateBytes;
    B_TRY(b->syStates.alloc((size_t) nItems * (size_t) b->stateBytes));
    b->scratchBytes = (b->sy->scratch_bytes(b->ringD) + (b->fused ? b->sy->fx_scratch_bytes(b->ringD) : 0) + 63) / 64 * 64;
    B_TRY(b->syScratch.alloc((size_t) nItems * (size_t) b->scratchBytes));
    B_TRY(b->track.alloc((size_t) plan.trackTotal * (size_t) b->trackRow));
    B_TRY(b->trackBase.alloc((size_t) nItems));
    B_TRY(hipMemcpyAsync(b->trackBase.p, plan.trackBase.data(), (size_t) nItems * sizeof(long long),
                         hipMemcpyHostToDevice, c->prep));
    B_TRY(hipStreamSynchronize(c->prep));
    lap("state, scratch, track allocation");
    return CPECAN_OK;
}

/* The hand-scheduled assembly sweeps, for a batch the kernel choice found fit for them (Dispatch::asmSweeps) and
 * that runs as one stream group on the one ring format, where the module loads: the plan, the forward waves'
 * contexts, the masks. */
static int asm_setup(cpecan_batch *b, const BandPlan &plan, const Dispatch &d, Lap &lap) {
    cpecan_ctx *c = b->ctx;
    const int64_t nItems = b->nItems;
    const AsmFormat f = asm_format(d.asmCells); /* (of the batch's cells per lane) */
    if (!d.asmSweeps || b->nGroups != 1 || b->stateBytes != (int) sizeof(WvState) ||
        b->sy->ringRowDoubles * 8 != f.rowBytes /* (one ring format) */ || cpecan_asm_load(c->device) != 0)
        return CPECAN_OK;
    b->asmMaxWindows = std::max(plan.maxWindows, 1);
    {
        PinnedBuf<AsmPlanWin> hWin;
        StreamFence winFence{ c->prep, nullptr };
        B_TRY(hWin.alloc((size_t) nItems * (size_t) b->asmMaxWindows));
        memset(hWin.p, 0, (size_t) nItems * (size_t) b->asmMaxWindows * sizeof(AsmPlanWin));
        for (int64_t i = 0; i < nItems; i++)
            std::copy(plan.asmWins[(size_t) i].begin(), plan.asmWins[(size_t) i].end(), hWin.p + (size_t) i * (size_t) b->asmMaxWindows);
        B_TRY(b->planWin.alloc(hWin.n));
        B_TRY(b->planCtl.alloc((size_t) plan.asmCtlTotal));
        B_TRY(b->planOff.alloc((size_t) nItems));
        B_TRY(b->asmCtx.alloc((size_t) nItems * 3 * (size_t) f.ctxBytes));
        B_TRY(b->asmMasks.alloc((size_t) (plan.diagTotal + 2) * (ASM_MASK_BYTES / 4)));
        B_TRY(hipMemsetAsync(b->asmMasks.p + (size_t) plan.diagTotal * (ASM_MASK_BYTES / 4), 0, 2 * ASM_MASK_BYTES, c->prep));
        B_TRY(hipMemcpyAsync(b->planWin.p, hWin.p, hWin.n * sizeof(AsmPlanWin), hipMemcpyHostToDevice, c->prep));
        B_TRY(hipMemcpyAsync(b->planCtl.p, plan.asmCtl.p, (size_t) plan.asmCtlTotal * sizeof(AsmPlanCtl), hipMemcpyHostToDevice, c->prep));
        B_TRY(hipMemcpyAsync(b->planOff.p, plan.asmOff.data(), (size_t) nItems * sizeof(long long), hipMemcpyHostToDevice, c->prep));
        hipError_t asmErr = cpecan_asm_launch_masks(c->prep, b->items.p, nItems, plan.maxDiags, b->bandTab.p, b->asmMasks.p,
                                                    f.cells);
        if (asmErr == hipSuccess)
            asmErr = cpecan_asm_launch_ctx_init(c->prep, b->items.p, nItems, b->asmCtx.p, f.ctxBytes, b->Fstore.p,
                                                b->ringDoubles, b->ringD, f.cells);
        B_TRY(hipStreamSynchronize(c->prep)); /* hWin ends here */
        if (asmErr != hipSuccess) {
            /* the compiled kernels need none of this: the batch runs on them (cpecan_hip_batch_assembly_sweeps
             * reports 0 and leaves the reason in last_error) */
            b->asmSetupError = std::string("assembly sweeps not set up: ") + hipGetErrorString(asmErr);
            if (getenv("CPECAN_ASM_TRACE")) fprintf(stderr, "[cpecan asm] %s\n", b->asmSetupError.c_str());
            return CPECAN_OK;
        }
    }
    if (b->ringD >= 3 * plan.maxSpan + 8 || plan.maxWindows <= 2) {
        /* the post kernel of a window runs beside the next window's sweeps (enqueue_sweeps, cpecan_run.hip): the sweep back of window
         * w+1 fills one half of the scratch while the post kernel of window w reads the other */
        B_TRY(b->syScratch.alloc(2 * (size_t) nItems * (size_t) b->scratchBytes));
        b->postAside = true;
        b->evPost.assign((size_t) b->asmMaxWindows, nullptr);
        for (auto &e : b->evPost) B_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    b->useAsm = true;
    b->asmCells = f.cells;
    b->asmBackward = d.asmBackward;
    if (getenv("CPECAN_ASM_TRACE"))
        fprintf(stderr, "[cpecan asm] batch of %lld alignments, widest band %d, %d windows: assembly sweeps, %d cells per lane\n",
                (long long) nItems, b->maxWidth, b->asmMaxWindows, b->asmCells);
    lap("assembly sweeps: plan upload, contexts");
    return CPECAN_OK;
}

/* what the kernels read per X position, part of input preparation (done once, like H2D): k-mer indices, or k-mer ids
 * over the HDP's alphabet */
static int index_kmers(cpecan_batch *b, int64_t nX) {
    cpecan_ctx *c = b->ctx;
    const XSource x = MACHINES[b->machine].x;
    const int blocks = (int) ((nX + 255) / 256);
    if (x == X_KID) {
        unsigned long long lo = 0, hi = 0;
        for (size_t q = 0; q < c->hdpAlphabet.size(); q++) {
            const unsigned long long ch = (unsigned char) c->hdpAlphabet[q];
            if (q < 8) lo |= ch << (8 * q);
            else hi |= ch << (8 * (q - 8));
        }
        B_TRY(b->kid.alloc((size_t) nX + 8));
        if (blocks > 0)
            hipLaunchKernelGGL(cpecan_k_hdp_kmer_id, dim3(blocks), dim3(256), 0, c->prep,
                               (const char *) b->chars.p, (long long) nX, lo, hi, (int) c->hdpAlphabet.size(),
                               b->kid.p);
    } else if (x == X_KIDX && blocks > 0)
        hipLaunchKernelGGL(cpecan_k_kmer_index, dim3(blocks), dim3(256), 0, c->prep,
                           (const char *) b->chars.p, (long long) nX, b->kidx.p);
    B_TRY(hipGetLastError());
    B_TRY(hipStreamSynchronize(c->prep)); /* every upload of batch creation has landed */
    return CPECAN_OK;
}

/* events != NULL: k-mers against events with a signal machine; yChars != NULL: DNA against DNA with the 5-state symbol
 * machine (nEvents then counts the bases of yChars) */
static int batch_create_impl(cpecan_ctx *c, Machine machine, const cpecan_item *items, int64_t nItems,
                             const char *xChars, int64_t nX, const double *events, const char *yChars,
                             int64_t nEvents, const int64_t *anchors, int64_t nAnchorPairs,
                             const cpecan_band_params *params, int32_t mode, int32_t kernel,
                             int32_t flags, cpecan_batch **out) {
    const MachineRow &m = MACHINES[machine];
    if (!c || !items || nItems <= 0 || !xChars || (machine == DNA5 ? !yChars : !events) || !params || !out)
        return fail(CPECAN_EINVAL, "bad argument");
    int rc = check_machine(machine, mode, flags);
    if (rc != CPECAN_OK) return rc;
    if (nAnchorPairs > 0 && !anchors) return fail(CPECAN_EINVAL, "anchors is NULL");
    if (params->diagonalExpansion < 0 || (params->diagonalExpansion & 1) ||
        params->traceBackDiagonals < 1 || params->minDiagsBetweenTraceBack < 2 ||
        params->traceBackDiagonals + 1 >= params->minDiagsBetweenTraceBack)
        return fail(CPECAN_EINVAL, "banding parameters violate the prerequisites of "
                                   "getPosteriorProbsWithBanding (pairwiseAligner.c:880-884)");
    *out = nullptr;
    HIP_TRY(hipSetDevice(c->device));
    const BatchInput in = { items, nItems, xChars, nX, events, yChars, nEvents, anchors, nAnchorPairs, params, mode,
                            (flags & CPECAN_FLAG_UNBANDED) != 0 };
    /* what the kernel choice comes to before the bands are known: its refusals, whether the general kernel's tables
     * are wanted at once, whether the assembly sweeps' plan is */
    DispatchQuery q = { machine, mode, kernel, flags, 0, true, read_batch_env() };
    const Dispatch early = choose_dispatch(q);
    if (early.refusal != CPECAN_OK) return fail(early.refusal, "%s", early.why);

    Lap lap("batch_create");
    BandPlan plan;
    StreamFence prepFence{ c->prep, nullptr }; /* (the plan's pinned blocks are uploaded through it) */
    if ((rc = check_items(c, machine, in, plan)) != CPECAN_OK) return rc;
    if ((rc = plan_bands(in, m, early, plan)) != CPECAN_OK) return rc;
    lap("band construction and window schedule (host)");
    q.maxWidth = plan.maxWidth;
    q.edgesStepByOne = plan.edgesStepByOne;
    q.noKmer = machine == VANILLA && vanilla_meets_no_kmer(in);
    const Dispatch d = choose_dispatch(q);
    if (d.refusal != CPECAN_OK) return fail(d.refusal, "%s", d.why);

    cpecan_batch *b = new_batch(c, machine, in, plan, d);
    if (!b) return fail(CPECAN_EINVAL, "out of host memory");
    /* every block from here on is the batch's (a step that fails destroys it, and its account is empty again) */
    MemScope mem(b->mem);
    if ((rc = upload_sequences(b, in)) != CPECAN_OK) return rc;
    lap("upload sequences and events");
    if ((rc = alloc_outputs(b, plan)) != CPECAN_OK) return rc;
    lap("output buffers");
    if (d.kernel == CPECAN_KERNEL_GENERAL) rc = general_storage(b, in, plan);
    else if ((rc = sweep_storage(b, plan, d, q.env, lap)) == CPECAN_OK) rc = asm_setup(b, plan, d, lap);
    if (rc != CPECAN_OK) return rc;
    B_TRY(hipEventCreate(&b->ev0));
    B_TRY(hipEventCreate(&b->ev1));
    B_TRY(hipEventCreate(&b->ev2));
    if ((rc = index_kmers(b, nX)) != CPECAN_OK) return rc;
    lap("k-mer index kernel");
    *out = b;
    return CPECAN_OK;
}

extern "C" {

int cpecan_hip_batch_create(cpecan_ctx *c, const cpecan_item *items, int64_t nItems,
                            const char *xChars, int64_t nX, const double *events, int64_t nEvents,
                            const int64_t *anchors, int64_t nAnchorPairs,
                            const cpecan_band_params *params, int32_t mode, int32_t kernel,
                            int32_t flags, cpecan_batch **out) {
    return batch_create_impl(c, STRAWMAN, items, nItems, xChars, nX, events, nullptr, nEvents, anchors, nAnchorPairs,
                             params, mode, kernel, flags, out);
}

int cpecan_hip_batch_create_vanilla(cpecan_ctx *c, const cpecan_item *items, int64_t nItems,
                                    const char *xChars, int64_t nX, const double *events, int64_t nEvents,
                                    const int64_t *anchors, int64_t nAnchorPairs,
                                    const cpecan_band_params *params, int32_t flags, cpecan_batch **out) {
    return batch_create_impl(c, VANILLA, items, nItems, xChars, nX, events, nullptr, nEvents, anchors, nAnchorPairs, params,
                             (flags & CPECAN_FLAG_EXPECTATIONS) ? CPECAN_MODE_EXPECTATIONS : CPECAN_MODE_POSTERIOR,
                             CPECAN_KERNEL_AUTO, flags & ~CPECAN_FLAG_EXPECTATIONS, out);
}

int cpecan_hip_batch_create_hdp(cpecan_ctx *c, const cpecan_item *items, int64_t nItems,
                                const char *xChars, int64_t nX, const double *events, int64_t nEvents,
                                const int64_t *anchors, int64_t nAnchorPairs,
                                const cpecan_band_params *params, int32_t flags, cpecan_batch **out) {
    return batch_create_impl(c, HDP, items, nItems, xChars, nX, events, nullptr, nEvents, anchors, nAnchorPairs, params,
                             (flags & CPECAN_FLAG_EXPECTATIONS) ? CPECAN_MODE_EXPECTATIONS : CPECAN_MODE_POSTERIOR,
                             CPECAN_KERNEL_AUTO, flags & ~CPECAN_FLAG_EXPECTATIONS, out);
}

int cpecan_hip_batch_create_dna(cpecan_ctx *c, const cpecan_item *items, int64_t nItems,
                                const char *xChars, int64_t nX, const char *yChars, int64_t nY,
                                const int64_t *anchors, int64_t nAnchorPairs,
                                const cpecan_band_params *params, int32_t flags, cpecan_batch **out) {
    return batch_create_impl(c, DNA5, items, nItems, xChars, nX, nullptr, yChars, nY, anchors, nAnchorPairs, params,
                             (flags & CPECAN_FLAG_EXPECTATIONS) ? CPECAN_MODE_EXPECTATIONS : CPECAN_MODE_POSTERIOR,
                             CPECAN_KERNEL_GENERAL, flags & ~CPECAN_FLAG_EXPECTATIONS, out);
}

int cpecan_hip_batch_create_sm4(cpecan_ctx *c, const cpecan_item *items, int64_t nItems, const char *xChars, int64_t nX,
                                const double *events, int64_t nEvents, const int64_t *anchors, int64_t nAnchorPairs,
                                const cpecan_band_params *params, int32_t flags, cpecan_batch **out) {
    if (flags & CPECAN_FLAG_EXPECTATIONS) return fail(CPECAN_EINVAL, "4-state batches: posterior decode only");
    return batch_create_impl(c, SM4, items, nItems, xChars, nX, events, nullptr, nEvents, anchors, nAnchorPairs, params,
                             CPECAN_MODE_POSTERIOR, CPECAN_KERNEL_GENERAL, flags, out);
}

int cpecan_hip_batch_create_echelon(cpecan_ctx *c, const cpecan_item *items, int64_t nItems, const char *xChars,
                                    int64_t nX, const double *events, int64_t nEvents, const int64_t *anchors,
                                    int64_t nAnchorPairs, const cpecan_band_params *params, int32_t flags,
                                    cpecan_batch **out) {
    if (flags & CPECAN_FLAG_EXPECTATIONS)
        return fail(CPECAN_EINVAL, "echelon batches: posterior decode only (the reference has no expectations for this machine)");
    return batch_create_impl(c, ECHELON, items, nItems, xChars, nX, events, nullptr, nEvents, anchors, nAnchorPairs, params,
                             CPECAN_MODE_POSTERIOR, CPECAN_KERNEL_GENERAL, flags, out);
}

int cpecan_hip_batch_systolic_rows(cpecan_batch *b, int32_t *rows) {
    if (!b || !rows) return fail(CPECAN_EINVAL, "bad argument");
    if (b->kernel != CPECAN_KERNEL_SYSTOLIC) return fail(CPECAN_EINVAL, "not a systolic batch");
    *rows = b->sy->rows;
    return CPECAN_OK;
}

int cpecan_hip_batch_kernel_family(cpecan_batch *b, int32_t *wave) {
    if (!b || !wave) return fail(CPECAN_EINVAL, "bad argument");
    if (b->machine == DNA5) { /* the 5-state machine: one wave per alignment (cpecan_kernel_wave5.hip) where the choice fell on it */
        *wave = b->wave5 ? 1 : 0;
        return CPECAN_OK;
    }
    if (b->machine == SM4) { /* the 4-state machine likewise (cpecan_kernel_wave4.hip, CPECAN_FLAG_SM4_WAVE) */
        *wave = b->wave4 ? 1 : 0;
        return CPECAN_OK;
    }
    if (b->kernel != CPECAN_KERNEL_SYSTOLIC) return fail(CPECAN_EINVAL, "not a register-resident batch");
    *wave = b->sy->wave ? 1 : 0;
    return CPECAN_OK;
}

int cpecan_hip_batch_expectation_pass(cpecan_batch *b, int32_t *fused) {
    if (!b || !fused) return fail(CPECAN_EINVAL, "bad argument");
    *fused = b->fused ? 1 : 0; /* (the strawMan wave kernels' E-step, or a fused build's: _f<n>, _vf<n>, _hf<n>) */
    return CPECAN_OK;
}

int cpecan_hip_batch_assembly_sweeps(cpecan_batch *b, int32_t *sweeps) {
    if (!b || !sweeps) return fail(CPECAN_EINVAL, "bad argument");
    *sweeps = b->useAsm ? (b->asmBackward ? 2 : 1) : 0;
    if (!b->asmSetupError.empty()) g_err = b->asmSetupError;
    return CPECAN_OK;
}

int cpecan_hip_batch_info(cpecan_batch *b, int32_t *kernel, int32_t *workgroups, int32_t *maxWidth) {
    if (!b) return fail(CPECAN_EINVAL, "batch is NULL");
    if (kernel) *kernel = b->kernel;
    if (workgroups) *workgroups = b->kernel == CPECAN_KERNEL_GENERAL ? (int32_t) b->nItems : b->nWorkers;
    if (maxWidth) *maxWidth = b->maxWidth;
    return CPECAN_OK;
}

/* The question of the plan calls, asked as batch creation asks it: what the machine refuses, the kernel choice before
 * the bands are known (*early), then with them (*d).  A refusal leaves its code and text as creation would. */
static int plan_query(int32_t machine, int32_t mode, int32_t kernel, int32_t flags, int32_t maxWidth, int32_t edgesStepByOne,
                      Dispatch *early, Dispatch *d) {
    if (machine < 0 || machine >= N_MACHINES) return fail(CPECAN_EINVAL, "unknown machine %d", machine);
    if (maxWidth < 0) return fail(CPECAN_EINVAL, "bad argument");
    const int rc = check_machine((Machine) machine, mode, flags);
    if (rc != CPECAN_OK) return rc;
    DispatchQuery q = { (Machine) machine, mode, kernel, flags, 0, true, read_batch_env() };
    *early = choose_dispatch(q);
    if (early->refusal != CPECAN_OK) return fail(early->refusal, "%s", early->why);
    q.maxWidth = maxWidth;
    q.edgesStepByOne = edgesStepByOne != 0;
    *d = choose_dispatch(q);
    if (d->refusal != CPECAN_OK) return fail(d->refusal, "%s", d->why);
    return CPECAN_OK;
}

int cpecan_hip_plan_dispatch(int32_t machine, int32_t mode, int32_t kernel, int32_t flags, int32_t maxWidth,
                             int32_t edgesStepByOne, int32_t *kernelOut, int32_t *waveOut, int32_t *rowsOut,
                             int32_t *buildMaxWidthOut) {
    Dispatch early, d;
    const int rc = plan_query(machine, mode, kernel, flags, maxWidth, edgesStepByOne, &early, &d);
    if (rc != CPECAN_OK) return rc;
    if (kernelOut) *kernelOut = d.kernel;
    if (waveOut) *waveOut = d.wave5 || d.wave4 || (d.build && d.build->wave) ? 1 : 0;
    if (rowsOut) *rowsOut = d.build ? d.build->rows : 0;
    if (buildMaxWidthOut) *buildMaxWidthOut = d.build ? d.build->maxWidth : 0;
    return CPECAN_OK;
}

int cpecan_hip_plan_assembly_sweeps(int32_t machine, int32_t mode, int32_t kernel, int32_t flags, int32_t maxWidth,
                                    int32_t edgesStepByOne, int32_t *cellsPerLaneOut) {
    if (cellsPerLaneOut) *cellsPerLaneOut = 0;
    Dispatch early, d;
    if (plan_query(machine, mode, kernel, flags, maxWidth, edgesStepByOne, &early, &d) != CPECAN_OK) return 0;
    /* (the plan is made only where the early answer asked for it: the same answer for every band, as it stands) */
    const int cells = early.asmPlan ? d.asmCells : 0;
    if (cellsPerLaneOut) *cellsPerLaneOut = cells;
    return cells;
}

int cpecan_hip_plan_expectation_pass(int32_t machine, int32_t mode, int32_t kernel, int32_t flags, int32_t maxWidth,
                                     int32_t edgesStepByOne, int32_t *fusedOut) {
    if (fusedOut) *fusedOut = 0;
    Dispatch early, d;
    if (plan_query(machine, mode, kernel, flags, maxWidth, edgesStepByOne, &early, &d) != CPECAN_OK) return 0;
    if (fusedOut) *fusedOut = d.fused ? 1 : 0;
    return d.fused ? 1 : 0;
}

} /* extern "C" */
