/*
 * stream_plan_test.c -- the chunking rule of the stream (csrc/host/cpecan_stream_plan.c) from a plain C program: built
 * from that one file and this one, with the address and undefined-behaviour sanitizers where the compiler has them
 * (tests/test_stream_plan_cpu.py builds and runs it).  Pseudo-random (class, cells) sequences and limits; every read
 * must land in exactly one chunk, a chunk holds one class, at most maxReads reads and -- past its first read -- at most
 * the budget's cells, reads keep their order inside a chunk, and with oneClass the chunks follow submission order.
 */
#include "cpecan_api.h"

#include <stdio.h>
#include <stdlib.h>

static uint64_t state = 0x9E3779B97F4A7C15ull;
static uint64_t next_random(void) { /* xorshift64 */
    state ^= state << 13;
    state ^= state >> 7;
    state ^= state << 17;
    return state;
}

static int check_case(int64_t n, int32_t nClasses, int64_t maxReads, int64_t budget, int32_t oneClass) {
    int32_t *cls = calloc((size_t) n + 1, sizeof(int32_t));
    int64_t *cells = calloc((size_t) n + 1, sizeof(int64_t)), *chunkOf = calloc((size_t) n + 1, sizeof(int64_t));
    int64_t *rankOf = calloc((size_t) n + 1, sizeof(int64_t));
    for (int64_t i = 0; i < n; i++) {
        cls[i] = (int32_t) (next_random() % (uint64_t) nClasses);
        cells[i] = 1 + (int64_t) (next_random() % 1000);
        chunkOf[i] = -1;
    }
    const int64_t nChunks = cpecan_stream_plan_chunks(n, cls, cells, maxReads, budget, oneClass, chunkOf, rankOf);
    int bad = 0;
    int64_t *count = calloc((size_t) nChunks + 1, sizeof(int64_t)), *sum = calloc((size_t) nChunks + 1, sizeof(int64_t));
    int64_t *first = malloc(sizeof(int64_t) * (size_t) (nChunks + 1));
    for (int64_t i = 0; i < n && !bad; i++) {
        const int64_t c = chunkOf[i];
        if (c < 0 || c >= nChunks) { bad = 1; break; }               /* every read in exactly one chunk */
        if (count[c] == 0) first[c] = i;
        else if (!oneClass && cls[first[c]] != cls[i]) bad = 2;       /* one class per chunk */
        if (rankOf[i] != count[c]) bad = 7;                          /* the chunk holds its reads in submission order */
        count[c]++;
        sum[c] += cells[i];
        if (count[c] > maxReads) bad = 3;
        if (count[c] > 1 && sum[c] > budget) bad = 4;
        if (oneClass && i > 0 && chunkOf[i] < chunkOf[i - 1]) bad = 5; /* submission order */
    }
    for (int64_t c = 0; c < nChunks && !bad; c++)
        if (count[c] == 0) bad = 6;
    if (bad) fprintf(stderr, "n %lld classes %d maxReads %lld budget %lld oneClass %d: rule %d broken\n", (long long) n,
                     nClasses, (long long) maxReads, (long long) budget, oneClass, bad);
    free(cls); free(cells); free(chunkOf); free(rankOf); free(count); free(sum); free(first);
    return bad;
}

int main(void) {
    int failures = 0;
    for (int k = 0; k < 300; k++) {
        const int64_t n = (int64_t) (next_random() % 200);
        const int32_t nClasses = 1 + (int32_t) (next_random() % 5);
        const int64_t maxReads = 1 + (int64_t) (next_random() % 12);
        const int64_t budget = 1 + (int64_t) (next_random() % 6000);
        failures += check_case(n, nClasses, maxReads, budget, (int32_t) (k % 3 == 0)) != 0;
    }
    failures += check_case(0, 1, 4, 100, 0) != 0;
    printf("stream plan: %d failures\n", failures);
    return failures ? 1 : 0;
}
