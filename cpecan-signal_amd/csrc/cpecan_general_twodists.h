/*
 * cpecan_general_twodists.h -- the inputs and emissions the vanilla and echelon general kernels share
 * (cpecan_kernel_generalv.hip, cpecan_kernel_generale.hip): X elements read as sequence_getKmer2 does
 * (impl/pairwiseAligner.c:320-325), the 30 skip bins of the k-mer pair (emissions_signal_getKmerSkipBin
 * impl/stateMachine.c:388), and emissions_signal_getEventMatchProbWithTwoDists (:499-528, logInvGaussPdf :322-331)
 * over a model block of the vanilla layout (cpecan_device.h: CP_VHDR, CP_VROW).
 */
#ifndef CPECAN_GENERAL_TWODISTS_H_
#define CPECAN_GENERAL_TWODISTS_H_

#include "cpecan_general.h"

template <int S_>
struct TwoDistCells : GeneralCells<S_> {
    const unsigned short *kidx; /* k-mer index per X character position (4096 = not a k-mer) */
    const double *ev;           /* events, 3 doubles each */
    const double *lnoise;       /* log(event noise), host libm */
    const double *hdr;          /* model header: scalars and per-bin log transition probabilities */
    const double *rows;         /* CP_VROW doubles per k-mer */

    __device__ TwoDistCells(const DevGeneralArgs &a, const DevItem &it, long long modelStride) : GeneralCells<S_>(a, it) {
        kidx = (const unsigned short *) a.x + it.xOff;
        ev = (const double *) a.y + 3 * it.yOff;
        lnoise = a.yAux + it.yOff;
        hdr = (const double *) a.models + (long long) it.model * modelStride;
        rows = hdr + CP_VHDR;
    }

    /* the two k-mers sequence_getKmer2 exposes for sequence index ix: a pointer to character
     * max(ix-1, 0); the skip bin looks at the k-mers at +0 and +1, the emission at the one at +1
     * (so sequence index 0 is scored with k-mer 1, as in the reference) */
    __device__ __forceinline__ void kmers_of(long long ix, int &kPrev, int &kCur) const {
        const long long p = ix > 0 ? ix - 1 : 0;
        kPrev = kidx[p];
        kCur = kidx[p + 1];
    }
    /* the 5 per-bin log transition probabilities of the machine's model block */
    __device__ __forceinline__ const double *bin_logs(int kPrev, int kCur) const {
        const double d = fabs(rows[(long long) kCur * CP_VROW + CP_V_MU] - rows[(long long) kPrev * CP_VROW + CP_V_MU]);
        long long bin = (long long) (d / 0.5);
        if (bin >= 30) bin = 29;
        return hdr + CP_VHDR_BINS + bin * 5;
    }
    /* emissions_signal_getEventMatchProbWithTwoDists on table `o` (0: match table, 6: extra-event table) */
    __device__ __forceinline__ double emit2(int k, long long iy, int o) const {
        const double *r = rows + (long long) k * CP_VROW + o;
        double mean, noise, lnz;
        if (iy >= 0) {
            mean = ev[3 * iy];
            noise = ev[3 * iy + 1];
            lnz = lnoise[iy];
        } else { /* NULLEVENT {-inf, 0} (:261): log(0) = -inf */
            mean = CP_NEG_INF;
            noise = 0.0;
            lnz = CP_NEG_INF;
        }
        const double level = cp_logGauss(mean, r[CP_V_MU], r[CP_V_SD], r[CP_V_K]);
        const double a = (noise - r[CP_V_NMU]) / r[CP_V_NMU];
        const double l_twoPi = 1.8378770664093453;
        const double nz = (r[CP_V_LLAMBDA] - l_twoPi - 3 * lnz - r[CP_V_LAMBDA] * a * a / noise) / 2;
        return level + nz;
    }
};

#endif
