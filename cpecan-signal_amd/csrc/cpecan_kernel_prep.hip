/*
 * cpecan_kernel_prep.hip -- what the throughput kernels need once per batch or once per library, whichever build of
 * cpecan_kernel_wave.hip or cpecan_kernel_systolic.hip sweeps the batch: compiled once.
 *
 *   - per X position the k-mer index (cpecan_k_kmer_index) or the k-mer id over an HDP's alphabet
 *     (cpecan_k_hdp_kmer_id): input preparation, launched by batch creation (cpecan_hip.hip);
 *   - the track kernels: per matrix column of every alignment the constants its k-mer brings to the sweeps, in the row
 *     format of the family and the machine (cpecan_k_track, cpecan_k_sy_track_hdp: CP_ROW doubles, the workgroup
 *     family's strawMan and HDP builds; cpecan_k_wv_track, cpecan_k_wv_track_hdp: CP_WV_ROW, the wave family's;
 *     cpecan_k_wv_track_vanilla: CP_WV_ROW_VANILLA, the vanilla builds of both families);
 *   - the counts kernels, which copy the results out of the per-alignment states (SyState: cpecan_k_sy_counts, WvState:
 *     cpecan_k_wv_counts);
 *   - the six SweepMachine records (cpecan_sweep.h) that name a machine's track and counts launchers on a family; every
 *     SweepBuild of the machine points at its record;
 *   - the division self-test and the shader clock of the last run.
 */
#include "cpecan_device.h"
#include "cpecan_sweep.h"

#include <algorithm>
#include <vector>

/* k-mer index of every position of the concatenated nucleotide buffer
 * (emissions_discrete_getKmerIndex impl/stateMachine.c:104-139): A,C,G,T = 0..3, most significant
 * first; any other character makes the 6-mer "not a k-mer" (index 4096 here, > 4096 there). */
extern "C" __global__ void cpecan_k_kmer_index(const char *chars, long long n, unsigned short *kidx) {
    long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int v = 0;
    bool ok = i + 5 < n;
    if (ok) {
        for (int j = 0; j < 6; j++) {
            char ch = chars[i + j];
            int b = ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : -1;
            if (b < 0) ok = false;
            v = v * 4 + (b & 3);
        }
    }
    kidx[i] = ok ? (unsigned short) v : (unsigned short) 4096;
}

/* k-mer id over the model's alphabet for every position of the concatenated nucleotide buffer
 * (kmer_id impl/nanopore_hdp.c:348-380: most significant character first); -1 where one of the six
 * characters is outside the alphabet (the reference exits there) or the buffer ends */
extern "C" __global__ void cpecan_k_hdp_kmer_id(const char *chars, long long n, unsigned long long alphabet,
                                                unsigned long long alphabetHi, int alphabetSize, int *kid) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    int v = 0;
    bool ok = i + 5 < n;
    if (ok) {
        for (int j = 0; j < 6; j++) {
            const char ch = chars[i + j];
            int d = -1;
            for (int a = 0; a < alphabetSize; a++) {
                const char ac = (char) ((a < 8 ? alphabet >> (8 * a) : alphabetHi >> (8 * (a - 8))) & 0xff);
                if (ac == ch) d = a;
            }
            if (d < 0) ok = false;
            v = v * alphabetSize + (d < 0 ? 0 : d);
        }
    }
    kid[i] = ok ? v : -1;
}

/* The five track kernels: blocks along y take the alignments (grid.y is capped at 65535), threads along x the entries
 * i = x * row + j of an alignment's track, matrix column x = 0..lX.  (The loop is typed out in each of them: handed to
 * one inline function as a lambda, the same source compiles to other instructions.) */

/* workgroup family, strawMan: row x = model row of the k-mer that matrix column x scores (column 0 = the "not a k-mer"
 * sentinel, sequence_getKmer index -1, :314-318) */
extern "C" __global__ void cpecan_k_track(const DevItem *__restrict__ items, long long nItems,
                                          const long long *__restrict__ trackBase,
                                          const unsigned short *__restrict__ kidx,
                                          const double *__restrict__ models, double *track) {
    for (long long item = blockIdx.y; item < nItems; item += gridDim.y) { /* grid.y is capped at 65535 */
        const DevItem it = items[item];
        const double *rows = models + (long long) it.model * CP_MODEL_STRIDE + CP_MODEL_HEADER;
        const long long n = (it.lX + 1) * CP_ROW;
        double *dst = track + trackBase[item] * CP_ROW;
        for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n;
             i += (long long) gridDim.x * blockDim.x) {
            const long long x = i / CP_ROW;
            const int j = (int) (i - x * CP_ROW);
            const int k = x == 0 ? 4096 : (int) kidx[it.xOff + x - 1];
            dst[i] = rows[(long long) k * CP_ROW + j];
        }
    }
}

/* workgroup family, HDP, in the strawMan row format: entry 0 of column x (0..lX) = the offset (in doubles) of the table
 * row of the k-mer that matrix column x scores -- sequence_getKmer3 (:327-331): column 0 (index -1) reads the first
 * k-mer, like column 1 -- or -1 where the column is no k-mer; entry CP_GAPX = the flat gap-X emission log(0.1)
 * (stateMachine.c:1347), which the sweep back adds to the transitions as it does a strawMan k-mer's; the rest unused */
extern "C" __global__ void cpecan_k_sy_track_hdp(const DevItem *__restrict__ items, long long nItems,
                                                 const long long *__restrict__ trackBase,
                                                 const int *__restrict__ kid, const DevHdpModel *__restrict__ models,
                                                 double *track) {
    for (long long item = blockIdx.y; item < nItems; item += gridDim.y) { /* grid.y is capped at 65535 */
        const DevItem it = items[item];
        const DevHdpModel &m = models[it.model];
        const long long n = (it.lX + 1) * CP_ROW;
        double *dst = track + trackBase[item] * CP_ROW;
        for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n;
             i += (long long) gridDim.x * blockDim.x) {
            const long long x = i / CP_ROW;
            const int j = (int) (i - x * CP_ROW);
            double v = 0.0;
            if (j == 0) {
                const int id = kid[it.xOff + (x > 0 ? x - 1 : 0)];
                v = id < 0 ? -1.0 : (double) ((long long) m.kmerRow[id] * m.gridLength);
            } else if (j == CP_GAPX) v = CP_HDP_GAPX;
            dst[i] = v;
        }
    }
}

/* wave family, strawMan: column x (0..lX) = the 16 emission constants of the k-mer that matrix column x scores
 * (column 0 = the "not a k-mer" sentinel, sequence_getKmer index -1, :314-318), its gap-X emission plus each of the
 * three transitions into gap X (the eP + tP of cell_calculate*), and the emission itself */
extern "C" __global__ void cpecan_k_wv_track(const DevItem *__restrict__ items, long long nItems,
                                             const long long *__restrict__ trackBase,
                                             const unsigned short *__restrict__ kidx,
                                             const double *__restrict__ models, double *track) {
    for (long long item = blockIdx.y; item < nItems; item += gridDim.y) { /* grid.y is capped at 65535 */
        const DevItem it = items[item];
        const double *model = models + (long long) it.model * CP_MODEL_STRIDE;
        const double *rows = model + CP_MODEL_HEADER;
        const long long n = (it.lX + 1) * CP_WV_ROW;
        double *dst = track + trackBase[item] * CP_WV_ROW;
        for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n;
             i += (long long) gridDim.x * blockDim.x) {
            const long long x = i / CP_WV_ROW;
            const int jj = (int) (i - x * CP_WV_ROW);
            const int k = x == 0 ? 4096 : (int) kidx[it.xOff + x - 1];
            const double *r = rows + (long long) k * CP_ROW;
            double v;
            if (jj < 16) v = r[jj];
            else if (jj == 16) v = r[CP_GAPX] + model[T_GAP_OPEN_X];
            else if (jj == 17) v = r[CP_GAPX] + model[T_GAP_EXTEND_X];
            else if (jj == 18) v = r[CP_GAPX] + model[T_GAP_SWITCH_TO_X];
            else v = r[CP_GAPX];
            dst[i] = v;
        }
    }
}

/* both families, vanilla: matrix column x scores the k-mer pair sequence_getKmer2 (impl/pairwiseAligner.c:320-325)
 * exposes for sequence index x - 1 -- a pointer to character max(x - 2, 0): the skip bin looks at the k-mers there
 * and one further, the emissions at the one further (columns 0, 1 and 2 all score k-mers 0 and 1, as in the
 * reference).  Row: per table (match, extra event) mu, sd, 1/sd, K, noise mean, 1/mean, lambda,
 * log(lambda) - log(2 pi); then the bin's five log transition probabilities (cpecan_models.hip: derive_vanilla) */
extern "C" __global__ void cpecan_k_wv_track_vanilla(const DevItem *__restrict__ items, long long nItems,
                                                     const long long *__restrict__ trackBase,
                                                     const unsigned short *__restrict__ kidx,
                                                     const double *__restrict__ models, double *track) {
    for (long long item = blockIdx.y; item < nItems; item += gridDim.y) { /* grid.y is capped at 65535 */
        const DevItem it = items[item];
        const double *hdr = models + (long long) it.model * CP_VMODEL_STRIDE;
        const double *rows = hdr + CP_VHDR;
        const long long n = (it.lX + 1) * CP_WV_ROW_VANILLA;
        double *dst = track + trackBase[item] * CP_WV_ROW_VANILLA;
        for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n;
             i += (long long) gridDim.x * blockDim.x) {
            const long long x = i / CP_WV_ROW_VANILLA;
            const int jj = (int) (i - x * CP_WV_ROW_VANILLA);
            const long long p = x > 2 ? x - 2 : 0;
            const int kPrev = kidx[it.xOff + p], kCur = kidx[it.xOff + p + 1];
            const double *r = rows + (long long) kCur * CP_VROW;
            double v = 0.0;
            if (jj < 16) {
                const double *q = r + 6 * (jj >> 3);
                switch (jj & 7) {
                case 0: v = q[CP_V_MU]; break;
                case 1: v = q[CP_V_SD]; break;
                case 2: v = q[CP_V_SD] == 0.0 ? 0.0 : 1.0 / q[CP_V_SD]; break;
                case 3: v = q[CP_V_K]; break;
                case 4: v = q[CP_V_NMU]; break;
                case 5: v = 1.0 / q[CP_V_NMU]; break;
                case 6: v = q[CP_V_LAMBDA]; break;
                default: v = q[CP_V_LLAMBDA] - 1.8378770664093453; break;
                }
            } else {
                const double d = fabs(r[CP_V_MU] - rows[(long long) kPrev * CP_VROW + CP_V_MU]);
                long long bin = (long long) (d / 0.5);
                if (bin >= 30) bin = 29;
                v = jj < 21 ? hdr[CP_VHDR_BINS + bin * 5 + (jj - 16)] : (double) bin; /* (entry 21: the bin itself, E-step) */
            }
            dst[i] = v;
        }
    }
}

/* wave family, HDP: column x (0..lX) = the offset (in doubles) of the table row of the k-mer that matrix
 * column x scores -- sequence_getKmer3 (:327-331): column 0 (index -1) reads the first k-mer, like column 1 -- and
 * the flat gap-X emission log(0.1) (stateMachine.c:1347) plus each of the three transitions into gap X */
extern "C" __global__ void cpecan_k_wv_track_hdp(const DevItem *__restrict__ items, long long nItems,
                                                 const long long *__restrict__ trackBase,
                                                 const int *__restrict__ kid, const DevHdpModel *__restrict__ models,
                                                 double *track) {
    for (long long item = blockIdx.y; item < nItems; item += gridDim.y) { /* grid.y is capped at 65535 */
        const DevItem it = items[item];
        const DevHdpModel &m = models[it.model];
        const long long n = (it.lX + 1) * CP_WV_ROW;
        double *dst = track + trackBase[item] * CP_WV_ROW;
        const double px = CP_HDP_GAPX;
        for (long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x; i < n;
             i += (long long) gridDim.x * blockDim.x) {
            const long long x = i / CP_WV_ROW;
            const int jj = (int) (i - x * CP_WV_ROW);
            double v = 0.0;
            if (jj == 0) {
                const int id = kid[it.xOff + (x > 0 ? x - 1 : 0)];
                v = id < 0 ? -1.0 : (double) ((long long) m.kmerRow[id] * m.gridLength);
            } else if (jj == 16) v = px + m.t[T_GAP_OPEN_X];
            else if (jj == 17) v = px + m.t[T_GAP_EXTEND_X];
            else if (jj == 18) v = px + m.t[T_GAP_SWITCH_TO_X];
            else if (jj == 19) v = px;
            dst[i] = v;
        }
    }
}

/* results of the per-alignment states into the batch's count arrays */
extern "C" __global__ void cpecan_k_sy_counts(const SyState *states, long long nItems,
                                              long long *nPairs, long long *nTot, long long *nCells) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nItems) return;
    nPairs[i] = states[i].nPairs;
    nTot[i] = states[i].nTot;
    nCells[i] = states[i].cells;
}
extern "C" __global__ void cpecan_k_wv_counts(const WvState *states, long long nItems, long long *nPairs,
                                              long long *nTot, long long *nCells) {
    const long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nItems) return;
    nPairs[i] = states[i].nPairs;
    nTot[i] = states[i].nTot;
    nCells[i] = states[i].cells;
}

/* division self-test (see cpecan_hip_selftest_division) */
extern "C" __global__ void cpecan_k_divtest(long long n, unsigned long long seed, unsigned long long *bad) {
    long long i = (long long) blockIdx.x * blockDim.x + threadIdx.x;
    unsigned long long local = 0;
    for (; i < n; i += (long long) gridDim.x * blockDim.x) {
        unsigned long long z = seed + 0x9E3779B97F4A7C15ull * (unsigned long long) (i + 1);
        double u[3];
        for (int k = 0; k < 3; k++) { /* splitmix64 */
            z += 0x9E3779B97F4A7C15ull;
            unsigned long long r = z;
            r = (r ^ (r >> 30)) * 0xBF58476D1CE4E5B9ull;
            r = (r ^ (r >> 27)) * 0x94D049BB133111EBull;
            r ^= r >> 31;
            u[k] = (double) (r >> 11) * (1.0 / 9007199254740992.0);
        }
        const bool noise = (i & 1) != 0;
        const double x = noise ? 0.001 + 4.0 * u[0] : 30.0 + 70.0 * u[0];
        const double mu = noise ? 0.3 + 2.0 * u[1] : 40.0 + 45.0 * u[1];
        const double sd = noise ? 0.05 + 1.5 * u[2] : 0.3 + 4.0 * u[2];
        const double rsd = 1.0 / sd;
        const double t = x - mu;
        const double q = t * rsd;
        const double rem = __fma_rn(-q, sd, t);
        const double a = __fma_rn(rem, rsd, q);
        const double ref = t / sd;
        if (!(a == ref)) local++;
    }
    if (local) atomicAdd(bad, local);
}

static int prep_status() { return hipGetLastError() == hipSuccess ? 0 : -1; }

extern "C" int cpecan_systolic_divtest(hipStream_t stream, long long n, unsigned long long seed,
                                       unsigned long long *bad) {
    hipLaunchKernelGGL(cpecan_k_divtest, dim3(1024), dim3(256), 0, stream, n, seed, bad);
    return prep_status();
}

/* the shader clock the forward sweeps of the last run saw, in MHz (s_memtime ticks over 100 MHz s_memrealtime ticks,
 * summed over the first alignments of the batch); 0 when nothing ran */
extern "C" int cpecan_wave_shader_clock_mhz(hipStream_t stream, const void *states, long long nItems, double *mhz) {
    const long long n = nItems < 64 ? nItems : 64;
    std::vector<WvState> h((size_t) n);
    if (hipMemcpyAsync(h.data(), states, (size_t) n * sizeof(WvState), hipMemcpyDeviceToHost, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess)
        return -1;
    double c = 0, r = 0;
    for (const WvState &s : h) {
        c += (double) s.clkShader;
        r += (double) s.clkRef;
    }
    *mhz = r > 0 ? 100.0 * c / r : 0.0;
    return 0;
}

/* The launchers of a pass's first and last stage (the C-ABI layer sequences them: track, then per window the sweeps of
 * the batch's SweepBuild, then counts).  A track launcher is its kernel, the row that kernel writes, what the kernel
 * reads per X position and the state record the family's sweeps keep per alignment, which it clears. */
template <typename State, int ROW, typename Kernel, typename X, typename Model>
static int launch_track(Kernel kernel, const X *x, const Model *models, hipStream_t stream, const SweepArgs &a) {
    const long long bx = (((long long) a.maxLX + 1) * ROW + 255) / 256;
    hipLaunchKernelGGL(kernel, dim3((unsigned) std::min(bx, 64LL), (unsigned) std::min(a.nItems, 65535LL)), dim3(256), 0,
                       stream, a.items, a.nItems, a.trackBase, x, models, a.track);
    if (hipMemsetAsync(a.states, 0, (size_t) a.nItems * sizeof(State), stream) != hipSuccess) return -1;
    return prep_status();
}
static int sy_launch_track(hipStream_t stream, const SweepArgs &a) {
    return launch_track<SyState, CP_ROW>(cpecan_k_track, a.kidx, a.models, stream, a);
}
static int sy_launch_track_vanilla(hipStream_t stream, const SweepArgs &a) {
    return launch_track<SyState, CP_WV_ROW_VANILLA>(cpecan_k_wv_track_vanilla, a.kidx, a.models, stream, a);
}
static int sy_launch_track_hdp(hipStream_t stream, const SweepArgs &a) {
    return launch_track<SyState, CP_ROW>(cpecan_k_sy_track_hdp, a.kid, (const DevHdpModel *) a.models, stream, a);
}
static int wv_launch_track(hipStream_t stream, const SweepArgs &a) {
    return launch_track<WvState, CP_WV_ROW>(cpecan_k_wv_track, a.kidx, a.models, stream, a);
}
static int wv_launch_track_vanilla(hipStream_t stream, const SweepArgs &a) {
    return launch_track<WvState, CP_WV_ROW_VANILLA>(cpecan_k_wv_track_vanilla, a.kidx, a.models, stream, a);
}
static int wv_launch_track_hdp(hipStream_t stream, const SweepArgs &a) {
    return launch_track<WvState, CP_WV_ROW>(cpecan_k_wv_track_hdp, a.kid, (const DevHdpModel *) a.models, stream, a);
}
static int sy_launch_counts(hipStream_t stream, const SweepArgs &a) {
    hipLaunchKernelGGL(cpecan_k_sy_counts, dim3((unsigned) ((a.nItems + 255) / 256)), dim3(256), 0, stream,
                       (const SyState *) a.states, a.nItems, a.nPairs, a.nTot, a.nCells);
    return prep_status();
}
static int wv_launch_counts(hipStream_t stream, const SweepArgs &a) {
    hipLaunchKernelGGL(cpecan_k_wv_counts, dim3((unsigned) ((a.nItems + 255) / 256)), dim3(256), 0, stream,
                       (const WvState *) a.states, a.nItems, a.nPairs, a.nTot, a.nCells);
    return prep_status();
}

/* the records (host only: the device pass would emit them as constants, with pointers to host functions) */
#ifndef __HIP_DEVICE_COMPILE__
const SweepMachine cpecan_systolic_machine = { (int) sizeof(SyState), CP_ROW, sy_launch_track, sy_launch_counts };
const SweepMachine cpecan_systolic_machine_vanilla = { (int) sizeof(SyState), CP_WV_ROW_VANILLA, sy_launch_track_vanilla,
                                                       sy_launch_counts };
const SweepMachine cpecan_systolic_machine_hdp = { (int) sizeof(SyState), CP_ROW, sy_launch_track_hdp, sy_launch_counts };
const SweepMachine cpecan_wave_machine = { (int) sizeof(WvState), CP_WV_ROW, wv_launch_track, wv_launch_counts };
const SweepMachine cpecan_wave_machine_vanilla = { (int) sizeof(WvState), CP_WV_ROW_VANILLA, wv_launch_track_vanilla,
                                                   wv_launch_counts };
const SweepMachine cpecan_wave_machine_hdp = { (int) sizeof(WvState), CP_WV_ROW, wv_launch_track_hdp, wv_launch_counts };
#endif
