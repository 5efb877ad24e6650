/*
 * cpecan_kernel_generalv.hip -- banded forward / backward / posterior DP for the reference's
 * 3-state "vanilla" signal machine (stateMachine3Vanilla_cellCalculate, impl/stateMachine.c:1368-1409;
 * SURVEY R12): transition probabilities that depend on the reference position through 30 skip bins
 * (emissions_signal_getBetaOrAlphaSkipProb :421, getKmerSkipBin :388), Gaussian level + inverse-
 * Gaussian noise emissions (emissions_signal_getEventMatchProbWithTwoDists :499-528,
 * logInvGaussPdf :322-331), X elements read as sequence_getKmer2 does (impl/pairwiseAligner.c:320-325).
 *
 * On the general driver (cpecan_general.h): any band width, posterior decode and Baum-Welch
 * expectations.  The inputs and the emission are shared with the echelon kernel (cpecan_general_twodists.h).
 *
 * Every log() the reference takes per cell is a function of the skip bin, the k-mer or the event
 * alone, so the host takes them once with its libm (cpecan_models.hip: derive_vanilla); the device
 * adds them in the reference's order.
 */
#include "cpecan_general_twodists.h"

namespace {

__device__ __forceinline__ double match_fromv(const double *middle, double eP, const double *bl, const double *hdr) {
    double m = CP_NEG_INF;
    m = cp_logAdd(m, middle[0] + (eP + bl[2]));               /* log a_mm */
    m = cp_logAdd(m, middle[1] + (eP + bl[3]));               /* log a_xm */
    m = cp_logAdd(m, middle[2] + (eP + hdr[CP_VHDR_LOG_YM])); /* log a_ym */
    return m;
}

struct Vanilla : TwoDistCells<3> {
    static constexpr bool kExpect = true;
    double (*sExp)[CP_EXPECTV_LEN + 1]; /* the E-step's sums in LDS, one copy per wave */

    long long lX;

    __device__ Vanilla(const DevGeneralArgs &a, const DevItem &it, double (*sExp_)[CP_EXPECTV_LEN + 1])
        : TwoDistCells<3>(a, it, CP_VMODEL_STRIDE), sExp(sExp_), lX(it.lX) {}

    /* TwoDistCells::kmers_of within the item's own sequence: a k-mer that starts at or past character lX runs into the
     * terminator of the reference's string and is no k-mer there (an item of no or one k-mer reads such a one) */
    __device__ __forceinline__ void kmers_of(long long ix, int &kPrev, int &kCur) const {
        const long long p = ix > 0 ? ix - 1 : 0;
        kPrev = p < lX ? (int) kidx[p] : 4096;
        kCur = p + 1 < lX ? (int) kidx[p + 1] : 4096;
    }

    __device__ __forceinline__ double match_into(const double *middle, long long x, long long y) const {
        int kPrev, kCur;
        kmers_of(x - 1, kPrev, kCur);
        return match_fromv(middle, emit2(kCur, y - 1, 0), bin_logs(kPrev, kCur), hdr);
    }

    /* stateMachine3_startStateProb / raggedStartStateProb (:1168-1177), shared with sm3 */
    __device__ __forceinline__ void start_vector(bool ragged, double e[3]) const {
        e[0] = ragged ? CP_NEG_INF : 0.0;
        e[1] = ragged ? 0.0 : CP_NEG_INF;
        e[2] = ragged ? 0.0 : CP_NEG_INF;
    }
    /* stateMachine3Vanilla_endStateProb / raggedEndStateProb (:1209-1235) */
    __device__ __forceinline__ void end_vector(bool ragged, double e[3]) const {
        const double eM = hdr[CP_VHDR_END_M], eX = hdr[CP_VHDR_END_X], eY = hdr[CP_VHDR_END_Y];
        e[0] = ragged ? (eX + eY) / 2.0 : eM;
        e[1] = eX;
        e[2] = eY;
    }

    /* cell_calculateForward over stateMachine3Vanilla_cellCalculate */
    __device__ __forceinline__ void forward_cell(long long d, int xmy, double o[3]) const {
        const long long x = (d + xmy) / 2, y = (d - xmy) / 2;
        int kPrev, kCur;
        kmers_of(x - 1, kPrev, kCur);
        const double *bl = bin_logs(kPrev, kCur);
        o[0] = o[1] = o[2] = CP_NEG_INF;
        const double *lower = fcell(d - 1, xmy - 1);
        const double *middle = fcell(d - 2, xmy);
        const double *upper = fcell(d - 1, xmy + 1);
        if (lower) {
            o[1] = cp_logAdd(o[1], lower[0] + (0 + bl[0])); /* log a_mx */
            o[1] = cp_logAdd(o[1], lower[1] + (0 + bl[1])); /* log a_xx */
        }
        if (middle) o[0] = match_fromv(middle, emit2(kCur, y - 1, 0), bl, hdr);
        if (upper) {
            const double eP = emit2(kCur, y - 1, 6);
            o[2] = cp_logAdd(o[2], upper[0] + (eP + bl[4]));                 /* log a_my */
            o[2] = cp_logAdd(o[2], upper[2] + (eP + hdr[CP_VHDR_LOG_YY])); /* log a_yy */
        }
    }

    /* gather form of cell_calculateBackward, the reference's scatter order kept per target state */
    __device__ __forceinline__ void backward_cell(long long d, long long dTop, int xmy, double o[3]) const {
        const long long x = (d + xmy) / 2, y = (d - xmy) / 2;
        o[0] = o[1] = o[2] = CP_NEG_INF;
        /* (ii) cell (x+1, y+1) on d+2, its middle block: its X element is index x, its event index y */
        const double *s2 = bcell(d + 2, dTop, xmy);
        if (s2) {
            int kPrev, kCur;
            kmers_of(x, kPrev, kCur);
            const double *bl = bin_logs(kPrev, kCur);
            const double eP = emit2(kCur, y, 0);
            o[0] = cp_logAdd(o[0], s2[0] + (eP + bl[2]));
            o[1] = cp_logAdd(o[1], s2[0] + (eP + bl[3]));
            o[2] = cp_logAdd(o[2], s2[0] + (eP + hdr[CP_VHDR_LOG_YM]));
        }
        /* (iii) cell (x, y+1) on d+1, its upper block: X element x-1, event y */
        const double *su = bcell(d + 1, dTop, xmy - 1);
        if (su) {
            int kPrev, kCur;
            kmers_of(x - 1, kPrev, kCur);
            const double *bl = bin_logs(kPrev, kCur);
            const double eP = emit2(kCur, y, 6);
            o[0] = cp_logAdd(o[0], su[2] + (eP + bl[4]));
            o[2] = cp_logAdd(o[2], su[2] + (eP + hdr[CP_VHDR_LOG_YY]));
        }
        /* (iv) cell (x+1, y) on d+1, its lower block: X element x */
        const double *sl = bcell(d + 1, dTop, xmy + 1);
        if (sl) {
            int kPrev, kCur;
            kmers_of(x, kPrev, kCur);
            const double *bl = bin_logs(kPrev, kCur);
            o[0] = cp_logAdd(o[0], sl[1] + (0 + bl[0]));
            o[1] = cp_logAdd(o[1], sl[1] + (0 + bl[1]));
        }
    }

    /* diagonalCalculation_Expectations :841-863 with cell_signal_updateBetaAndAlphaProb :478-498:
     * of all transitions only match->gapX (into the cell's skip bin) and gapX->gapX (bin + 30)
     * are collected; both live in the lower block */
    __device__ __forceinline__ void expect_diagonal(const DevGeneralArgs &, const DevParams &, const DevItem &,
                                                    long long d2, int l2, int w2, const double *bdd, double total,
                                                    bool, long long &) const {
        const int tid = threadIdx.x, wave = tid >> 6;
        double *acc = sExp[wave];
        if (tid == 0) acc[CP_EXPECTV_LEN - 1] += total;
        for (int cc = tid; cc < w2; cc += 256) {
            const int xmy = l2 + 2 * cc;
            const long long x = (d2 + xmy) / 2;
            const double *lower = fcell(d2 - 1, xmy - 1);
            if (!lower) continue;
            int kPrev, kCur;
            kmers_of(x - 1, kPrev, kCur);
            const double *bl = bin_logs(kPrev, kCur);
            const int bin = (int) ((bl - (hdr + CP_VHDR_BINS)) / 5);
            const double *cur = bdd + cc * 3;
            atomicAdd(&acc[bin], exp(lower[0] + cur[1] + (0 + bl[0]) - total));
            atomicAdd(&acc[bin + 30], exp(lower[1] + cur[1] + (0 + bl[1]) - total));
        }
    }
    __device__ __forceinline__ void expect_fold(const DevGeneralArgs &a, const DevItem &it) const {
        __syncthreads();
        double *dst = a.expect + (long long) it.model * CP_EXPECTV_LEN;
        for (int i = threadIdx.x; i < CP_EXPECTV_LEN; i += 256) {
            const double v = ((sExp[0][i] + sExp[1][i]) + sExp[2][i]) + sExp[3][i];
            if (v != 0.0) atomicAdd(dst + i, v);
        }
    }
};

} // namespace

extern "C" __global__ __launch_bounds__(256) void cpecan_k_generalv(DevGeneralArgs a, DevParams P) {
    /* Baum-Welch sums of this alignment (VanillaHmm): 30 beta + 30 alpha skip bins and the likelihood,
     * one copy per wave, folded into the model's block of `expect` at the end */
    __shared__ double sExp[4][CP_EXPECTV_LEN + 1];
    for (int i = threadIdx.x; i < 4 * (CP_EXPECTV_LEN + 1); i += 256) (&sExp[0][0])[i] = 0.0;
    const DevItem it = a.items[blockIdx.x];
    Vanilla m(a, it, sExp);
    general_pass(m, a, P, it);
}
