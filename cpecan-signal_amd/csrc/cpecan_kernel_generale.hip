/*
 * cpecan_kernel_generale.hip -- banded forward / backward / posterior DP for the reference's echelon signal machine
 * (stateMachineEchelon_cellCalculate, impl/stateMachine.c:1411-1455; stateMachineEchelon_construct :1602-1640;
 * getStateMachineEchelon :1773): match states match0..match5 for an event that covers 0..5 k-mers and a k-mer skip
 * state gapX.  The transitions come from the vanilla machine's 30 skip bins (beta, alpha; emissions_signal_
 * getBetaOrAlphaSkipProb :421) and a Poisson posterior of the event's duration (emissions_signal_getDurationProb
 * :551, poissonPosteriorProb :345-370); the emissions are the two-distribution ones of the vanilla machine
 * (cpecan_general_twodists.h), summed over n k-mers for match_n (emissions_signal_multipleKmerMatchProb :530-549).
 *
 * On the general driver (cpecan_general.h): any band width; the backward recurrence is the gather form of the
 * reference's scatter, contributions added in the reference's order per target state.  Posterior decode only, with
 * diagonalCalculationMultiPosteriorMatchProbs (impl/pairwiseAligner.c:797-839): the reference passes no expectation
 * function for this machine.
 *
 * Every log() the reference takes per cell is one of the skip bin (log beta, log alpha, log(1-beta), log(1-alpha)),
 * the k-mer, the event (log noise, the six duration terms) or n (log n): the host takes them with its libm
 * (cpecan_models.hip: derive_echelon; cpecan_hip.hip: batch creation) and the device adds them in the reference's order.
 *
 * Quirks kept: the end state vector is {0.790..., 0.196...} used as log values (:1620, "these aren't log"); the sum of
 * multipleKmerMatchProb starts from 0.0, not log zero; its only look-ahead is whether the character 6n places after
 * the getKmer2 pointer is upper case -- past the sequence that is the pad 'n' of sequence_padSequence.
 */
#include "cpecan_general_twodists.h"

namespace {

enum { E_GAPX = 6 }; /* match0..match5 = 0..5, gapX = 6 (impl/stateMachine.c:1165) */
enum { E_LB = 0, E_LA = 1, E_L1B = 2, E_L1A = 3 }; /* a bin's log beta, log alpha, log(1-beta), log(1-alpha) */

struct Echelon : TwoDistCells<7> {
    static constexpr bool kMultiMatch = true;
    const char *xc;       /* this item's X characters */
    long long xEnd;       /* characters from xc on that belong to the sequence; the rest read as the pad 'n' */
    const double *dur;    /* 6 per event: the duration terms of 0..5 k-mers */
    const double *logn;   /* log(n), n = 0..5 */

    __device__ Echelon(const DevGeneralArgs &a, const DevEchelonArgs &e, const DevItem &it)
        : TwoDistCells<7>(a, it, CP_EMODEL_STRIDE) {
        xc = e.xChars + it.xOff;
        xEnd = e.xEnd[blockIdx.x];
        dur = e.yDur + 6 * it.yOff;
        logn = hdr + CP_EMODEL_LOGN;
    }

    /* emissions_signal_multipleKmerMatchProb (:530-549) of cX = sequence_getKmer2(X, ix), event iy, n k-mers */
    __device__ __forceinline__ double multi(long long ix, long long iy, int n) const {
        const long long p = ix > 0 ? ix - 1 : 0;
        const long long q = p + 6 * n;
        const char c = q < xEnd ? xc[q] : 'n';
        if (!(c >= 'A' && c <= 'Z')) return CP_NEG_INF;
        double s = 0.0;
        for (int i = 0; i < n; i++) s = cp_logAdd(s, emit2(kidx[p + 1 + i], iy, 0));
        return s - logn[n];
    }
    /* the middle block (:1432-1444): match0..5 and gapX of (x-1, y-1) into match1..5, in the reference's call order */
    __device__ __forceinline__ void middle_into(const double *middle, long long ix, long long iy, const double *bl,
                                                double o[S]) const {
        double eP[6];
#pragma unroll
        for (int n = 1; n < 6; n++) {
            eP[n] = multi(ix, iy, n);
            const double tP = bl[E_L1B] + dur[6 * iy + n];
#pragma unroll
            for (int from = 0; from < 6; from++) o[n] = cp_logAdd(o[n], middle[from] + (eP[n] + tP));
        }
#pragma unroll
        for (int n = 1; n < 6; n++) o[n] = cp_logAdd(o[n], middle[E_GAPX] + (eP[n] + (bl[E_L1A] + dur[6 * iy + n])));
    }
    __device__ __forceinline__ void step_into(const double *middle, long long x, long long y, double o[S]) const {
        int kPrev, kCur;
        kmers_of(x - 1, kPrev, kCur);
        middle_into(middle, x - 1, y - 1, bin_logs(kPrev, kCur), o);
    }

    /* stateMachineEchelon_startStateProb / raggedStartStateProb (:1237-1246) */
    __device__ __forceinline__ void start_vector(bool ragged, double e[S]) const {
#pragma unroll
        for (int s = 0; s < S; s++) e[s] = CP_NEG_INF;
        if (ragged) e[E_GAPX] = 0.0;
        else e[1] = 0.0;
    }
    /* stateMachineEchelon_endStateProb, also its ragged end (:1248-1262, :1629-1630) */
    __device__ __forceinline__ void end_vector(bool, double e[S]) const {
#pragma unroll
        for (int s = 0; s < 6; s++) e[s] = hdr[CP_VHDR_END_M];
        e[E_GAPX] = hdr[CP_VHDR_END_X];
    }

    /* cell_calculateForward (impl/pairwiseAligner.c:365-375) over stateMachineEchelon_cellCalculate */
    __device__ __forceinline__ void forward_cell(long long d, int xmy, double o[S]) const {
        const long long x = (d + xmy) / 2, y = (d - xmy) / 2;
        int kPrev, kCur;
        kmers_of(x - 1, kPrev, kCur);
        const double *bl = bin_logs(kPrev, kCur);
#pragma unroll
        for (int s = 0; s < S; s++) o[s] = CP_NEG_INF;
        const double *lower = fcell(d - 1, xmy - 1);
        const double *middle = fcell(d - 2, xmy);
        const double *upper = fcell(d - 1, xmy + 1);
        if (lower) {
#pragma unroll
            for (int n = 1; n < 6; n++) o[E_GAPX] = cp_logAdd(o[E_GAPX], lower[n] + (0 + bl[E_LB]));
            o[E_GAPX] = cp_logAdd(o[E_GAPX], lower[E_GAPX] + (0 + bl[E_LA]));
        }
        if (middle) middle_into(middle, x - 1, y - 1, bl, o);
        if (upper) {
            const double eP = emit2(kCur, y - 1, 6), tP = bl[E_L1B] + dur[6 * (y - 1)];
#pragma unroll
            for (int n = 1; n < 6; n++) o[0] = cp_logAdd(o[0], upper[n] + (eP + tP));
        }
    }

    /* gather form of cell_calculateBackward (:378-389): what reaches this cell from the cell above-right on d+2 (its
     * middle block), from (x, y+1) on d+1 (its upper block) and from (x+1, y) on d+1 (its lower block), in that order;
     * within a block in the order of stateMachineEchelon_cellCalculate's calls */
    __device__ __forceinline__ void backward_cell(long long d, long long dTop, int xmy, double o[S]) const {
        const long long x = (d + xmy) / 2, y = (d - xmy) / 2;
#pragma unroll
        for (int s = 0; s < S; s++) o[s] = CP_NEG_INF;
        const double *s2 = bcell(d + 2, dTop, xmy);
        if (s2) { /* X element x, event y */
            int kPrev, kCur;
            kmers_of(x, kPrev, kCur);
            const double *bl = bin_logs(kPrev, kCur);
            double eP[6];
#pragma unroll
            for (int n = 1; n < 6; n++) {
                eP[n] = multi(x, y, n);
                const double tP = bl[E_L1B] + dur[6 * y + n];
#pragma unroll
                for (int from = 0; from < 6; from++) o[from] = cp_logAdd(o[from], s2[n] + (eP[n] + tP));
            }
#pragma unroll
            for (int n = 1; n < 6; n++) o[E_GAPX] = cp_logAdd(o[E_GAPX], s2[n] + (eP[n] + (bl[E_L1A] + dur[6 * y + n])));
        }
        const double *su = bcell(d + 1, dTop, xmy - 1);
        if (su) { /* X element x-1, event y */
            int kPrev, kCur;
            kmers_of(x - 1, kPrev, kCur);
            const double *bl = bin_logs(kPrev, kCur);
            const double eP = emit2(kCur, y, 6), tP = bl[E_L1B] + dur[6 * y];
#pragma unroll
            for (int n = 1; n < 6; n++) o[n] = cp_logAdd(o[n], su[0] + (eP + tP));
        }
        const double *sl = bcell(d + 1, dTop, xmy + 1);
        if (sl) { /* X element x */
            int kPrev, kCur;
            kmers_of(x, kPrev, kCur);
            const double *bl = bin_logs(kPrev, kCur);
#pragma unroll
            for (int n = 1; n < 6; n++) o[n] = cp_logAdd(o[n], sl[E_GAPX] + (0 + bl[E_LB]));
            o[E_GAPX] = cp_logAdd(o[E_GAPX], sl[E_GAPX] + (0 + bl[E_LA]));
        }
    }
};

} // namespace

extern "C" __global__ __launch_bounds__(256) void cpecan_k_generale(DevGeneralArgs a, DevParams P, DevEchelonArgs e) {
    const DevItem it = a.items[blockIdx.x];
    Echelon m(a, e, it);
    general_pass(m, a, P, it);
}
