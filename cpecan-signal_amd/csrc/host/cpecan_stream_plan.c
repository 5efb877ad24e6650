/*
 * cpecan_stream_plan.c -- the chunking rule of the stream (cpecan_stream.c) as plain bookkeeping: no device, no thread,
 * nothing of the library beyond this file, so that a stand-alone program can be built from it (tests/c/stream_plan_test.c).
 *
 * Reads arrive one at a time, each with a class (the kernel it would run on alone) and a size in cells.  Every class has
 * one open group.  A read joins its class's group; if the group could not take it -- it would then hold more than
 * maxReads reads, or more cells than the budget the caller names for that class at that moment -- the group is closed
 * first and comes back to the caller as a chunk, and the read opens the class's next group.  A group takes its first
 * read whatever its size.  Flushing closes the open groups in the order in which they got their first read.  Reads keep
 * their order of arrival inside a group.
 */
#include "cpecan_host_private.h"

#include <stdlib.h>
#include <string.h>

void planner_init(StreamPlanner *pl, int64_t maxReads) {
    memset(pl, 0, sizeof *pl);
    pl->maxReads = maxReads < 1 ? 1 : maxReads;
}

static bool same_class(StreamClass a, StreamClass b) { return a.kernel == b.kernel && a.wave == b.wave && a.rows == b.rows; }

/* the group is handed over as it is (the caller frees its items array) and the class's group is empty again */
static void hand_over(StreamGroup *g, StreamGroup *closed) {
    *closed = *g;
    g->items = NULL;
    g->n = g->cap = g->cells = 0;
}

bool planner_add(StreamPlanner *pl, StreamClass cls, int64_t cells, int64_t cellBudget, void *item, StreamGroup *closed) {
    StreamGroup *g = NULL;
    for (int64_t k = 0; k < pl->nGroups && !g; k++)
        if (same_class(pl->groups[k].cls, cls)) g = &pl->groups[k];
    if (!g) {
        if (pl->nGroups == pl->capGroups) {
            pl->capGroups = pl->capGroups ? 2 * pl->capGroups : 8;
            pl->groups = realloc(pl->groups, sizeof(StreamGroup) * (size_t) pl->capGroups);
        }
        g = &pl->groups[pl->nGroups++];
        memset(g, 0, sizeof *g);
        g->cls = cls;
    }
    const bool closes = g->n > 0 && (g->n + 1 > pl->maxReads || g->cells + cells > cellBudget);
    if (closes) hand_over(g, closed);
    if (g->n == 0) g->opened = pl->opened++;
    if (g->n == g->cap) {
        g->cap = g->cap ? 2 * g->cap : 16;
        g->items = realloc(g->items, sizeof(void *) * (size_t) g->cap);
    }
    g->items[g->n++] = item;
    g->cells += cells;
    return closes;
}

bool planner_flush_one(StreamPlanner *pl, StreamGroup *closed) {
    StreamGroup *first = NULL;
    for (int64_t k = 0; k < pl->nGroups; k++)
        if (pl->groups[k].n > 0 && (!first || pl->groups[k].opened < first->opened)) first = &pl->groups[k];
    if (!first) return false;
    hand_over(first, closed);
    return true;
}

void planner_free(StreamPlanner *pl) {
    for (int64_t k = 0; k < pl->nGroups; k++) free(pl->groups[k].items);
    free(pl->groups);
    memset(pl, 0, sizeof *pl);
}

/* Test hook: the rule over n reads at once, with one cell budget for every class.  chunkOf[i] receives the chunk of read
 * i, chunks numbered in the order in which they close (the flush at the end included), rankOf[i] its place among that
 * chunk's reads as the chunk holds them; returns how many chunks there are. */
int64_t cpecan_stream_plan_chunks(int64_t n, const int32_t *classOf, const int64_t *cells, int64_t maxReadsPerChunk,
                                  int64_t cellBudget, int32_t oneClass, int64_t *chunkOf, int64_t *rankOf) {
    StreamPlanner pl;
    StreamGroup closed;
    int64_t nChunks = 0;
    planner_init(&pl, maxReadsPerChunk);
    for (int64_t i = 0; i <= n; i++) {
        bool got;
        if (i < n) {
            const StreamClass cls = { oneClass ? 0 : classOf[i], 0, 0 };
            got = planner_add(&pl, cls, cells[i], cellBudget, (void *) (intptr_t) (i + 1), &closed);
        } else
            got = planner_flush_one(&pl, &closed);
        while (got) {
            for (int64_t k = 0; k < closed.n; k++) {
                chunkOf[(intptr_t) closed.items[k] - 1] = nChunks;
                rankOf[(intptr_t) closed.items[k] - 1] = k;
            }
            free(closed.items);
            nChunks++;
            got = i == n && planner_flush_one(&pl, &closed);
        }
    }
    planner_free(&pl);
    return nChunks;
}
