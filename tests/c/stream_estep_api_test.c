/* Compiled against include/cpecan_api.h and include/cpecan_hip.h alone: the names this round added are declared with the
 * types a C caller relies on (assigning them to function pointers of those types is the check, under -Werror), and the
 * one of them that needs no device answers.  Prints the E-step class of a strawMan read of the width given. */
#include "cpecan_api.h"
#include "cpecan_hip.h"

#include <stdio.h>
#include <stdlib.h>

static void done(void *arg, int64_t tag, bool refused) {
    (void) arg; (void) tag; (void) refused;
}

int main(int argc, char **argv) {
    int (*sum)(cpecan_batch *, double *) = cpecan_hip_batch_sum_expectations;
    cpecan_stream *(*open)(PairwiseAlignmentParameters *, bool, bool, const cpecan_stream_options *, void *,
                           cpecan_stream_done_fn, cpecan_stream_chunk_fn, void *) = cpecan_stream_open_expectations;
    cpecan_stream_done_fn onDone = done;
    ContinuousPairHmmExpectations target; /* (what a strawMan stream would be opened with) */
    target.likelihood = 0.0;
    int32_t kernel = -1, wave = -1, rows = -1;
    const int rc = cpecan_stream_expectations_class(CPECAN_MACHINE_STRAWMAN, argc > 1 ? atoi(argv[1]) : 100, 1, &kernel,
                                                    &wave, &rows);
    if (!sum || !open || !onDone || rc != CPECAN_OK || target.likelihood != 0.0) return 1;
    printf("ok %d %d %d\n", kernel, wave, rows);
    return 0;
}
