/*
 * cpecan_band_extent.h -- the two facts about a band that the kernel choice asks for, taken diagonal by diagonal: how
 * many cells the diagonal holds and whether its edges moved by at most one matrix column from the diagonal before.
 * One rule for batch creation (build_bands, cpecan_hip.hip), which takes it inside its own pass over the band, and for
 * cpecan_band_extent (cpecan_geometry.c), which answers for one item without a batch; and the one fact about an item's
 * characters that the choice asks for, shared with the host library's stream (csrc/host/cpecan_stream.c).  Plain C.
 */
#ifndef CPECAN_BAND_EXTENT_H
#define CPECAN_BAND_EXTENT_H

#include <stdint.h>

/* Diagonal k with the x-y interval [L, R]: returns its cells, col receives its first and last matrix column; prev: the
 * columns of diagonal k-1 (not read for k = 0); *stepByOne is cleared where an edge moved back or by more than one. */
static inline int cpecan_diag_extent(int64_t k, int32_t L, int32_t R, const int prev[2], int col[2], int *stepByOne) {
    col[0] = (int) ((k + L) / 2);
    col[1] = (int) ((k + R) / 2);
    if (k >= 1 && (col[0] < prev[0] || col[0] > prev[0] + 1 || col[1] < prev[1] || col[1] > prev[1] + 1)) *stepByOne = 0;
    return ((R - L) >> 1) + 1;
}

/* Whether an item of the vanilla machine meets a k-mer that is none: a character outside ACGT among its lX + 5 (x: its
 * first), or fewer than two k-mers (sequence_getKmer2 looks one k-mer ahead, so an item of no or one k-mer reads the
 * k-mer that runs into its string's terminator).  Such an item runs on the general kernel (choose_dispatch). */
static inline int cpecan_item_meets_no_kmer(const char *x, int64_t lX) {
    if (lX < 2) return 1;
    for (int64_t k = 0; k < lX + 5; k++)
        if (x[k] != 'A' && x[k] != 'C' && x[k] != 'G' && x[k] != 'T') return 1;
    return 0;
}

#endif
