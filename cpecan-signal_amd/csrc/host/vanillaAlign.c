/*
 * vanillaAlign.c -- the signal-align driver of the reference (vanillaAlign.c:361-805) on top of libcpecan_host.so:
 * same command line, same inputs (a .npRead file, a reference sequence file, a guide alignment in exonerate CIGAR
 * format on stdin), same outputs (the 15-column TSV appended to --posteriors, the summary line on stdout, or the two
 * .expectations / .hmm files).  The template and the complement strand are aligned by two threads, as the
 * reference's two OpenMP sections do; each thread has a context of its own in the host library, so the two
 * alignments run on the GPU side by side.
 *
 * Not carried over: --buildHDP / --alignments (training and re-sampling HDPs is outside this path; the option is
 * refused with a message), and expectations or HMM files under the fourState and echelon machines (the reference has no
 * container for them either; its loadHmmRoutine refuses echelon, vanillaAlign.c:157).  The echelon machine aligns as the
 * reference's performSignalAlignmentP does: the target padded (sequence_padSequence, :197-199) and decoded with
 * diagonalCalculationMultiPosteriorMatchProbs (:236-238).
 *
 * The guide alignment comes through sonLib's cigarRead in the reference.  sonLib is not part of this build, so
 * the line format is read here directly: "cigar: <query> <qStart> <qEnd> <+|-> <target> <tStart> <tEnd> <+|-> <score>
 * {<M|I|D> <length>}...", query = the 2D read (contig2/start2/end2 in the reference's struct), target = the
 * reference sequence (contig1/start1/end1); M advances both, D the target only, I the query only.
 */
#include <dirent.h>
#include <getopt.h>
#include <math.h>
#include <pthread.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "cpecan_api.h"
#include "cpecan_hip.h" /* (the device cache's capacity, shared out between the two E-step streams) */

static void die(const char *fmt, ...) __attribute__((noreturn, format(printf, 1, 2)));
static void die(const char *fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vfprintf(stderr, fmt, ap);
    va_end(ap);
    fputc('\n', stderr);
    exit(1);
}

/* ---- the guide alignment ----------------------------------------------------------------------------------- */
typedef struct {
    char op; /* 'M', 'I' (query only), 'D' (target only) */
    int64_t length;
} CigarOp;
typedef struct {
    char contig1[256], contig2[256]; /* 1 = target (reference), 2 = query (read) */
    int64_t start1, end1, strand1, start2, end2, strand2;
    double score;
    CigarOp *ops;
    int64_t nOps;
} GuideAlignment;

static GuideAlignment *cigar_read(FILE *f) {
    GuideAlignment *pA = calloc(1, sizeof *pA);
    char s1, s2;
    long long a, b, c, d;
    if (fscanf(f, " cigar: %255s %lld %lld %c %255s %lld %lld %c %lf", pA->contig2, &a, &b, &s2, pA->contig1, &c, &d, &s1,
               &pA->score) != 9)
        die("vanillaAlign - ERROR: no guide alignment (exonerate cigar line) on stdin");
    pA->start2 = a; pA->end2 = b; pA->strand2 = s2 == '+';
    pA->start1 = c; pA->end1 = d; pA->strand1 = s1 == '+';
    int64_t cap = 16;
    pA->ops = malloc(sizeof(CigarOp) * (size_t) cap);
    char op;
    long long len;
    while (fscanf(f, " %c %lld", &op, &len) == 2) {
        if (op != 'M' && op != 'I' && op != 'D') die("vanillaAlign - ERROR: cigar operation '%c'", op);
        if (pA->nOps == cap) pA->ops = realloc(pA->ops, sizeof(CigarOp) * (size_t) (cap *= 2));
        pA->ops[pA->nOps].op = op;
        pA->ops[pA->nOps++].length = len;
    }
    return pA;
}
/* checkPairwiseAlignment: the operations account for both intervals */
static void cigar_check(const GuideAlignment *pA) {
    int64_t l1 = 0, l2 = 0;
    for (int64_t i = 0; i < pA->nOps; i++) {
        if (pA->ops[i].op != 'I') l1 += pA->ops[i].length;
        if (pA->ops[i].op != 'D') l2 += pA->ops[i].length;
    }
    if (l1 != llabs(pA->end1 - pA->start1) || l2 != llabs(pA->end2 - pA->start2))
        die("vanillaAlign - ERROR: the cigar's operations cover %lld / %lld positions, its intervals %lld / %lld",
            (long long) l1, (long long) l2, (long long) llabs(pA->end1 - pA->start1), (long long) llabs(pA->end2 - pA->start2));
}

static char complement_of(char c) {
    switch (c) {
    case 'A': return 'T'; case 'C': return 'G'; case 'G': return 'C'; case 'T': return 'A';
    case 'a': return 't'; case 'c': return 'g'; case 'g': return 'c'; case 't': return 'a';
    default: return c;
    }
}
static char *reverse_complement(const char *s) {
    const size_t n = strlen(s);
    char *r = malloc(n + 1);
    for (size_t i = 0; i < n; i++) r[i] = complement_of(s[n - 1 - i]);
    r[n] = 0;
    return r;
}
static char *substring(const char *s, int64_t start, int64_t length) {
    if (start < 0 || length < 0 || (size_t) (start + length) > strlen(s))
        die("vanillaAlign - ERROR: the guide alignment reaches outside the reference sequence");
    char *r = malloc((size_t) length + 1);
    memcpy(r, s + start, (size_t) length);
    r[length] = 0;
    return r;
}
static char *replace_char(const char *s, char from, const char *to) { /* stString_replace(s, "C", to) */
    const size_t lt = strlen(to);
    size_t n = 0;
    for (const char *p = s; *p; p++) n += *p == from ? lt : 1;
    char *r = malloc(n + 1), *q = r;
    for (const char *p = s; *p; p++) {
        if (*p == from) { memcpy(q, to, lt); q += lt; }
        else *q++ = *p;
    }
    *q = 0;
    return r;
}
static char *first_line(const char *path) {
    FILE *f = fopen(path, "r");
    if (!f) die("vanillaAlign - ERROR: cannot open %s", path);
    size_t cap = 1 << 16, n = 0;
    char *buf = malloc(cap);
    int ch;
    while ((ch = fgetc(f)) != EOF && ch != '\n') {
        if (n + 2 > cap) buf = realloc(buf, cap *= 2);
        buf[n++] = (char) ch;
    }
    buf[n] = 0;
    fclose(f);
    return buf;
}

/* guideAlignmentToRebasedAnchorPairs (vanillaAlign.c:278-298): the target interval re-based to 0 (and flipped to the
 * forward strand), match columns to (target, query) pairs with `trim` columns cut at both ends of every match block
 * (convertPairwiseForwardStrandAlignmentToAnchorPairs, impl/pairwiseAligner.c:1039-1063), sorted, overlap-filtered */
static stList *guide_to_anchor_pairs(GuideAlignment *pA, PairwiseAlignmentParameters *p) {
    const bool flip = !pA->strand1;
    const int64_t shift = pA->strand1 ? pA->start1 : pA->end1;
    pA->start1 -= shift;
    pA->end1 -= shift;
    if (flip) {
        pA->strand1 = !pA->strand1;
        const int64_t t = pA->end1;
        pA->end1 = pA->start1;
        pA->start1 = t;
    }
    cigar_check(pA);
    if (!pA->strand1 || !pA->strand2) die("vanillaAlign - ERROR: the read side of the guide alignment must be '+'");
    stList *pairs = stList_construct3(0, (void (*)(void *)) stIntTuple_destruct);
    int64_t j = pA->start1, k = pA->start2;
    for (int64_t i = 0; i < pA->nOps; i++) {
        const CigarOp *op = &pA->ops[i];
        if (op->op == 'M')
            for (int64_t l = p->constraintDiagonalTrim; l < op->length - p->constraintDiagonalTrim; l++)
                stList_append(pairs, stIntTuple_construct2(j + l, k + l));
        if (op->op != 'I') j += op->length;
        if (op->op != 'D') k += op->length;
    }
    stList_sort(pairs, stIntTuple_cmpFn);
    stList *filtered = filterToRemoveOverlap(pairs);
    stList_destruct(pairs);
    return filtered;
}

static Sequence *event_sequence_from_guide(double *events, int64_t queryStart, int64_t queryEnd, int64_t *eventMap) {
    const int64_t startIdx = eventMap[queryStart], endIdx = eventMap[queryEnd];
    if (endIdx < startIdx) /* the reference would build a Sequence of negative length here (vanillaAlign.c:300-314) */
        die("vanillaAlign - ERROR: the event map runs against the read (event %lld at read position %lld, %lld at %lld)",
            (long long) startIdx, (long long) queryStart, (long long) endIdx, (long long) queryEnd);
    return sequence_construct2(endIdx - startIdx, events + startIdx * NB_EVENT_PARAMS, sequence_getEvent,
                               sequence_sliceEventSequence2);
}

static StateMachine *build_state_machine(const char *modelFile, NanoporeReadAdjustmentParameters npp,
                                         StateMachineType type, Strand strand, NanoporeHDP *nHdp) {
    if (type == vanilla) {
        StateMachine *sM = getSignalStateMachine3Vanilla(modelFile);
        emissions_signal_scaleModel(sM, npp.scale, npp.shift, npp.var, npp.scale_sd, npp.var_sd);
        stateMachine3Vanilla_setStrandTransitionsToDefaults(sM, strand);
        return sM;
    }
    if (type == echelon) { /* vanillaAlign.c:127-130 */
        StateMachine *sM = getStateMachineEchelon(modelFile);
        emissions_signal_scaleModel(sM, npp.scale, npp.shift, npp.var, npp.scale_sd, npp.var_sd);
        return sM;
    }
    if (type == threeState || type == fourState) { /* vanillaAlign.c:104-140 */
        StateMachine *sM = type == fourState ? getStateMachine4(modelFile) : getStrawManStateMachine3(modelFile);
        emissions_signal_scaleModel(sM, npp.scale, npp.shift, npp.var, npp.scale_sd, npp.var_sd);
        return sM;
    }
    if (!nHdp) die("vanillaAlign - ERROR: the strawMan-HDP model needs --templateHdp and --complementHdp");
    return getHdpStateMachine3(nHdp);
}
static stList *remapped_anchor_pairs(stList *unmapped, int64_t *eventMap, int64_t mapOffset) {
    stList *remapped = nanopore_remapAnchorPairsWithOffset(unmapped, eventMap, mapOffset);
    stList *filtered = filterToRemoveOverlap(remapped);
    stList_destruct(remapped);
    return filtered;
}
static void *(*target_getter(StateMachineType type))(void *, int64_t) {
    return type == vanilla || type == echelon ? sequence_getKmer2 : type == threeStateHdp ? sequence_getKmer3 : sequence_getKmer;
}

/* ---- one strand: what one OpenMP section of the reference does ----------------------------------------------- */
typedef struct {
    /* in */
    Strand strand;
    StateMachineType type;
    const char *modelFile, *hmmFile, *expectationsFile, *posteriorProbsFile, *readLabel;
    NanoporeHDP *nHdp;
    NanoporeReadAdjustmentParameters npp;
    Sequence *eventSequence;
    double *allEvents;
    int64_t *eventMap, mapOffset, eventShift, referenceShift;
    char *target, *tsvTarget, *contig;
    bool forward;
    PairwiseAlignmentParameters *p;
    stList *anchorPairs;
    /* out */
    stList *alignedPairs;
    double posteriorScore;
    StateMachine *sM; /* kept for the TSV rows (the scaled match table) */
} StrandJob;

static void *strand_expectations(void *arg) { /* getSignalExpectations + hmmContinuous_writeToFile (:318-359, :680-716) */
    StrandJob *j = arg;
    const char *name = j->strand == template ? "template" : "complement";
    fprintf(stderr, "vanillaAlign - getting expectations for %s\n", name);
    Hmm *hmm = hmmContinuous_getEmptyHmm(j->type, 0.0001, j->p->threshold);
    StateMachine *sM = build_state_machine(j->modelFile, j->npp, j->type, j->strand, j->nHdp);
    if (j->hmmFile) {
        fprintf(stderr, "vanillaAlign - loading HMM from file, %s\n", j->hmmFile);
        hmmContinuous_loadSignalHmm(j->hmmFile, sM, j->type);
    }
    const int64_t lX = sequence_correctSeqLength((int64_t) strlen(j->target), event);
    stList *anchors = remapped_anchor_pairs(j->anchorPairs, j->eventMap, j->mapOffset);
    Sequence *target = sequence_construct2(lX, j->target, target_getter(j->type), sequence_sliceNucleotideSequence2);
    if (j->type == vanilla) vanillaHmm_implantMatchModelsintoHmm(sM, hmm);
    getExpectationsUsingAnchors(sM, hmm, target, j->eventSequence, anchors, j->p, diagonalCalculation_Expectations, 1, 1);
    fprintf(stderr, "vanillaAlign - writing expectations to file: %s\n", j->expectationsFile);
    if (j->type == threeStateHdp)
        fprintf(stderr, "vanillaAlign - got %lld HDP assignments\n", (long long) hmmContinuous_howManyAssignments(hmm));
    hmmContinuous_writeToFile(j->expectationsFile, hmm, j->type);
    hmmContinuous_destruct(hmm, j->type);
    sequence_sequenceDestroy(target);
    stList_destruct(anchors);
    stateMachine_destruct(sM);
    return NULL;
}

static void *strand_alignment(void *arg) { /* performSignalAlignment + writePosteriorProbs (:179-255, :737-790) */
    StrandJob *j = arg;
    fprintf(stderr, "vanillaAlign - starting %s alignment\n", j->strand == template ? "template" : "complement");
    StateMachine *sM = build_state_machine(j->modelFile, j->npp, j->type, j->strand, j->nHdp);
    if (j->hmmFile) {
        fprintf(stderr, "loading HMM from file, %s\n", j->hmmFile);
        hmmContinuous_loadSignalHmm(j->hmmFile, sM, sM->type);
    }
    const int64_t lX = sequence_correctSeqLength((int64_t) strlen(j->target), event);
    fprintf(stderr, "vanillaAlign - doing banded alignment\n");
    stList *anchors = remapped_anchor_pairs(j->anchorPairs, j->eventMap, j->mapOffset);
    Sequence *sX = sequence_construct2(lX, j->target, target_getter(j->type), sequence_sliceNucleotideSequence2);
    if (j->type == echelon) sequence_padSequence(sX);
    j->alignedPairs = getAlignedPairsUsingAnchors(sM, sX, j->eventSequence, anchors, j->p,
                                                  j->type == echelon ? diagonalCalculationMultiPosteriorMatchProbs
                                                                     : diagonalCalculationPosteriorMatchProbs, 1, 1);
    double total = 0.0; /* scoreByPosteriorProbabilityIgnoringGaps */
    for (int64_t i = 0; i < stList_length(j->alignedPairs); i++) total += (double) stIntTuple_get(stList_get(j->alignedPairs, i), 0);
    j->posteriorScore = 100.0 * total / ((double) stList_length(j->alignedPairs) * PAIR_ALIGNMENT_PROB_1);
    stList_sort(j->alignedPairs, sortByXPlusYCoordinate2);
    if (j->type == echelon) free(sX->elements); /* (the padded copy) */
    sequence_sequenceDestroy(sX);
    stList_destruct(anchors);
    j->sM = sM;
    return NULL;
}

/* ---- a directory of reads: what scripts/signalAlign.py does with a pool of vanillaAlign processes, one GPU batch here.
 * Every <name>.npRead of the directory is aligned with the guide alignment in <name>.cigar (the exonerate cigar line the
 * pipeline would pipe into the single-read driver); template and complement strands of all reads go through ONE call of
 * getAlignedPairsUsingAnchorsBatch; posteriors are written to <outDir>/<name>.tsv, the summary lines to stdout. --------- */
typedef struct {
    char *name, *trimmedRefSeq, *rcTrimmedRefSeq;
    NanoporeRead *npRead;
    GuideAlignment *pA;
    stList *anchorPairs;
    Sequence *events[2];
    int64_t nAnchors;
} BatchRead;

static int name_order(const void *a, const void *b) { return strcmp(*(char *const *) a, *(char *const *) b); }

/* the sorted names of the .npRead files of a directory (without the suffix) */
static char **read_names(const char *dir, int64_t *count) {
    DIR *d = opendir(dir);
    if (!d) die("vanillaAlign - ERROR: cannot open the directory %s", dir);
    char **names = NULL;
    int64_t n = 0, cap = 0;
    for (struct dirent *e; (e = readdir(d)) != NULL;) {
        const size_t l = strlen(e->d_name);
        if (l <= 7 || strcmp(e->d_name + l - 7, ".npRead") != 0) continue;
        if (n == cap) names = realloc(names, sizeof(char *) * (size_t) (cap = cap ? 2 * cap : 64));
        names[n] = malloc(l + 1);
        memcpy(names[n], e->d_name, l - 7);
        names[n++][l - 7] = 0;
    }
    closedir(d);
    if (n == 0) die("vanillaAlign - ERROR: no .npRead file in %s", dir);
    qsort(names, (size_t) n, sizeof(char *), name_order);
    fprintf(stderr, "vanillaAlign - %lld reads in %s\n", (long long) n, dir);
    *count = n;
    return names;
}

/* <dir>/<name>.npRead and its guide alignment <dir>/<name>.cigar: the read, the two targets, the event sequences, the anchors */
static void load_batch_read(BatchRead *r, const char *dir, char *name, const char *referenceSequence, StateMachineType sMtype,
                            PairwiseAlignmentParameters *p) {
    r->name = name;
    const size_t room = strlen(dir) + strlen(name) + 16;
    char *path = malloc(room);
    snprintf(path, room, "%s/%s.npRead", dir, name);
    r->npRead = nanopore_loadNanoporeReadFromFile(path);
    if (sMtype == threeStateHdp) nanopore_descaleNanoporeRead(r->npRead);
    snprintf(path, room, "%s/%s.cigar", dir, name);
    FILE *f = fopen(path, "r");
    if (!f) die("vanillaAlign - ERROR: no guide alignment %s", path);
    r->pA = cigar_read(f);
    fclose(f);
    free(path);
    GuideAlignment *pA = r->pA;
    r->trimmedRefSeq = pA->strand1 ? substring(referenceSequence, pA->start1, pA->end1 - pA->start1)
                                   : substring(referenceSequence, pA->end1, pA->start1 - pA->end1);
    if (!pA->strand1) {
        char *rc = reverse_complement(r->trimmedRefSeq);
        free(r->trimmedRefSeq);
        r->trimmedRefSeq = rc;
    }
    r->rcTrimmedRefSeq = reverse_complement(r->trimmedRefSeq);
    r->events[0] = event_sequence_from_guide(r->npRead->templateEvents, pA->start2, pA->end2, r->npRead->templateEventMap);
    r->events[1] = event_sequence_from_guide(r->npRead->complementEvents, pA->start2, pA->end2, r->npRead->complementEventMap);
    const int64_t start1 = pA->start1, end1 = pA->end1;
    const bool forward = pA->strand1;
    r->anchorPairs = guide_to_anchor_pairs(pA, p); /* (re-bases the target interval in pA) */
    r->nAnchors = stList_length(r->anchorPairs);
    pA->start1 = start1; /* the TSV rows need the original offsets */
    pA->end1 = end1;
    pA->strand1 = forward;
}

/* what one strand (0: template, 1: complement) of a loaded read is aligned with */
static void strand_inputs(BatchRead *r, int st, StateMachineType sMtype, const char *modelFiles[2], const char *hmmFiles[2],
                          NanoporeHDP *nHdps[2], StateMachine **sM, Sequence **sX, Sequence **sY, stList **anchors) {
    const NanoporeReadAdjustmentParameters npp = st == 0 ? r->npRead->templateParams : r->npRead->complementParams;
    *sM = build_state_machine(modelFiles[st], npp, sMtype, st == 0 ? template : complement, nHdps[st]);
    if (hmmFiles[st]) hmmContinuous_loadSignalHmm(hmmFiles[st], *sM, (*sM)->type);
    /* (as in the single-read driver, --substitute only applies when expectations are collected) */
    char *target = st == 0 ? r->trimmedRefSeq : r->rcTrimmedRefSeq;
    *sX = sequence_construct2(sequence_correctSeqLength((int64_t) strlen(target), event), target, target_getter(sMtype),
                              sequence_sliceNucleotideSequence2);
    *sY = r->events[st];
    *anchors = remapped_anchor_pairs(r->anchorPairs, st == 0 ? r->npRead->templateEventMap : r->npRead->complementEventMap,
                                     r->pA->start2);
}

/* the strand's rows appended to `out`; returns its score (scoreByPosteriorProbabilityIgnoringGaps) */
static double write_strand(const char *out, BatchRead *r, int st, StateMachine *sM, stList *pairs) {
    GuideAlignment *pA = r->pA;
    double total = 0.0;
    for (int64_t q = 0; q < stList_length(pairs); q++) total += (double) stIntTuple_get(stList_get(pairs, q), 0);
    const double score = 100.0 * total / ((double) stList_length(pairs) * PAIR_ALIGNMENT_PROB_1);
    stList_sort(pairs, sortByXPlusYCoordinate2);
    const NanoporeReadAdjustmentParameters npp = st == 0 ? r->npRead->templateParams : r->npRead->complementParams;
    const int64_t *map = st == 0 ? r->npRead->templateEventMap : r->npRead->complementEventMap;
    writePosteriorProbs((char *) out, r->name, sM->EMISSION_MATCH_PROBS, npp.scale, npp.shift,
                        st == 0 ? r->npRead->templateEvents : r->npRead->complementEvents,
                        st == 0 ? r->trimmedRefSeq : r->rcTrimmedRefSeq, pA->strand1, pA->contig1, map[pA->start2],
                        st == 0 ? pA->start1 : pA->end1, pairs, st == 0 ? template : complement);
    return score;
}

static char *tsv_path(const char *outDir, const char *name) {
    const size_t room = strlen(outDir) + strlen(name) + 16;
    char *out = malloc(room);
    snprintf(out, room, "%s/%s.tsv", outDir, name);
    return out;
}

static void free_batch_read(BatchRead *r) {
    if (r->events[0]) sequence_sequenceDestroy(r->events[0]);
    if (r->events[1]) sequence_sequenceDestroy(r->events[1]);
    if (r->anchorPairs) stList_destruct(r->anchorPairs);
    nanopore_nanoporeReadDestruct(r->npRead);
    free(r->pA->ops);
    free(r->pA);
    free(r->trimmedRefSeq);
    free(r->rcTrimmedRefSeq);
    free(r->name);
}

static int align_directory(const char *dir, const char *outDir, const char *referenceSequence, StateMachineType sMtype,
                           const char *modelFiles[2], const char *hmmFiles[2], NanoporeHDP *nHdps[2],
                           PairwiseAlignmentParameters *p, const char *substitute) {
    int64_t n;
    char **names = read_names(dir, &n);
    BatchRead *reads = calloc((size_t) n, sizeof(BatchRead));
    StateMachine **sMs = malloc(sizeof(StateMachine *) * 2 * (size_t) n);
    Sequence **sXs = malloc(sizeof(Sequence *) * 2 * (size_t) n), **sYs = malloc(sizeof(Sequence *) * 2 * (size_t) n);
    stList **anchors = malloc(sizeof(stList *) * 2 * (size_t) n);
    for (int64_t i = 0; i < n; i++) {
        load_batch_read(&reads[i], dir, names[i], referenceSequence, sMtype, p);
        for (int st = 0; st < 2; st++) {
            const int64_t k = 2 * i + st;
            strand_inputs(&reads[i], st, sMtype, modelFiles, hmmFiles, nHdps, &sMs[k], &sXs[k], &sYs[k], &anchors[k]);
        }
    }
    fprintf(stderr, "vanillaAlign - aligning %lld strands as one batch\n", (long long) (2 * n));
    stList **pairs = getAlignedPairsUsingAnchorsBatch(2 * n, sMs, sXs, sYs, anchors, p, 1, 1);
    for (int64_t i = 0; i < n; i++) {
        BatchRead *r = &reads[i];
        char *out = tsv_path(outDir, r->name);
        remove(out); /* (writePosteriorProbs appends) */
        double score[2];
        for (int st = 0; st < 2; st++) score[st] = write_strand(out, r, st, sMs[2 * i + st], pairs[2 * i + st]);
        fprintf(stdout, "%s %lld\t%lld(%f)\t%lld(%f)\n", r->name, (long long) r->nAnchors, (long long) stList_length(pairs[2 * i]),
                score[0], (long long) stList_length(pairs[2 * i + 1]), score[1]);
        free(out);
    }
    for (int64_t k = 0; k < 2 * n; k++) {
        stList_destruct(pairs[k]);
        stList_destruct(anchors[k]);
        sequence_sequenceDestroy(sXs[k]);
        stateMachine_destruct(sMs[k]);
    }
    (void) substitute;
    for (int64_t i = 0; i < n; i++) free_batch_read(&reads[i]);
    free(pairs); free(reads); free(sMs); free(sXs); free(sYs); free(anchors); free(names);
    fprintf(stderr, "vanillaAlign - SUCCESS: finished alignment of %lld reads, exiting\n", (long long) n);
    return 0;
}

/* ---- the same directory through the stream (--stream): reads are loaded, submitted and let go one at a time, the chunks
 * run chained within a device-memory budget, and a strand's rows are written when its result arrives.  What a strand's
 * rows are written from -- the read's events and event map, its two targets, its machine -- stays until both strands of
 * the read are written; the event sequences and anchor lists go as soon as the strands are submitted. ----------------- */
typedef struct {
    BatchRead r;
    StateMachine *sM[2];
    Sequence *sX[2];
    char *out, *summary; /* the TSV's path; the read's summary line, once both strands are written */
    stList *held;        /* the complement's pairs, where they arrived before the template's */
    int written, refused;
    int64_t nPairs[2];
    double score[2];
} StreamRead;
typedef struct {
    StreamRead *reads;
    int64_t nRefused;
} StreamDirectory;

static void stream_strand_done(StreamRead *sr, int st, stList *pairs) {
    sr->nPairs[st] = stList_length(pairs);
    sr->score[st] = write_strand(sr->out, &sr->r, st, sr->sM[st], pairs);
    stList_destruct(pairs);
    sr->written++;
}

/* (the stream never runs two of these at once) */
static void stream_result(void *arg, int64_t tag, stList *pairs) {
    StreamDirectory *sd = arg;
    StreamRead *sr = &sd->reads[tag / 2];
    const int st = (int) (tag % 2);
    if (!pairs) {
        fprintf(stderr, "vanillaAlign - ERROR: the %s strand of %s does not fit the device-memory budget, not aligned\n",
                st == 0 ? "template" : "complement", sr->r.name);
        sr->refused++;
        sd->nRefused++;
    } else if (st == 1 && sr->written == 0 && sr->refused == 0)
        sr->held = pairs; /* template first, as writePosteriorProbs appends them without --stream */
    else
        stream_strand_done(sr, st, pairs);
    if (sr->held && (sr->written == 1 || sr->refused)) {
        stList *held = sr->held;
        sr->held = NULL;
        stream_strand_done(sr, 1, held);
    }
    if (sr->written + sr->refused < 2) return;
    if (sr->written == 2) {
        const size_t room = strlen(sr->r.name) + 160;
        sr->summary = malloc(room);
        snprintf(sr->summary, room, "%s %lld\t%lld(%f)\t%lld(%f)\n", sr->r.name, (long long) sr->r.nAnchors,
                 (long long) sr->nPairs[0], sr->score[0], (long long) sr->nPairs[1], sr->score[1]);
    }
    for (int k = 0; k < 2; k++) {
        sequence_sequenceDestroy(sr->sX[k]);
        stateMachine_destruct(sr->sM[k]);
    }
    free(sr->out);
    free_batch_read(&sr->r);
}

static int align_directory_stream(const char *dir, const char *outDir, const char *referenceSequence, StateMachineType sMtype,
                                  const char *modelFiles[2], const char *hmmFiles[2], NanoporeHDP *nHdps[2],
                                  PairwiseAlignmentParameters *p, const cpecan_stream_options *options) {
    int64_t n;
    char **names = read_names(dir, &n);
    StreamDirectory sd = { calloc((size_t) n, sizeof(StreamRead)), 0 };
    cpecan_stream *stream = cpecan_stream_open(p, 1, 1, options, stream_result, NULL, &sd);
    for (int64_t i = 0; i < n; i++) {
        StreamRead *sr = &sd.reads[i];
        load_batch_read(&sr->r, dir, names[i], referenceSequence, sMtype, p);
        sr->out = tsv_path(outDir, names[i]);
        remove(sr->out); /* (writePosteriorProbs appends) */
        Sequence *sY[2];
        stList *anchors[2];
        for (int st = 0; st < 2; st++)
            strand_inputs(&sr->r, st, sMtype, modelFiles, hmmFiles, nHdps, &sr->sM[st], &sr->sX[st], &sY[st], &anchors[st]);
        /* (nothing of the read may be let go between the two: the template's result can arrive at once) */
        BatchRead *r = &sr->r;
        Sequence *events[2] = { r->events[0], r->events[1] };
        stList *anchorPairs = r->anchorPairs;
        r->events[0] = r->events[1] = NULL;
        r->anchorPairs = NULL;
        for (int st = 0; st < 2; st++) cpecan_stream_submit(stream, 2 * i + st, sr->sM[st], sr->sX[st], sY[st], anchors[st]);
        for (int st = 0; st < 2; st++) {
            stList_destruct(anchors[st]);
            sequence_sequenceDestroy(events[st]);
        }
        stList_destruct(anchorPairs);
    }
    int64_t nChunks = 0, nRefused = 0, peak = 0;
    cpecan_stream_close(stream, &nChunks, &nRefused, &peak);
    for (int64_t i = 0; i < n; i++) { /* in name order, as without --stream */
        if (sd.reads[i].summary) fputs(sd.reads[i].summary, stdout);
        free(sd.reads[i].summary);
    }
    free(sd.reads);
    free(names);
    fprintf(stderr, "vanillaAlign - stream: %lld chunks, at most %lld device bytes, %lld strands refused\n", (long long) nChunks,
            (long long) peak, (long long) nRefused);
    if (nRefused == 0) fprintf(stderr, "vanillaAlign - SUCCESS: finished alignment of %lld reads, exiting\n", (long long) n);
    return nRefused == 0 ? 0 : 1;
}

/* ---- the E-step over the directory (--stream with --templateExpectations / --complementExpectations): what
 * scripts/trainModels.py gets from one vanillaAlign process per read and a sum over their files, from two expectation
 * streams here, one per strand, each with half the budget and an accumulator of its own.  Reads are loaded, submitted and
 * let go one at a time; the targets carry the substitution, as the single-read E-step's do.  Of a read only its two state
 * machines stay, until its expectations are in. ---------------------------------------------------------------------- */
#define ESTEP_PSEUDOCOUNT 0.0001 /* the single-read driver's, per strand submitted: what the sum over per-read files holds */
typedef struct {
    const char *strand;
    char **names;
    StateMachine **sMs; /* per read */
    bool keepFirst;     /* the vanilla file carries the match tables of the first read in name order */
    int64_t nRefused;
} EstepStrands;

/* (a stream never runs two of these at once, and each stream has its own EstepStrands) */
static void estep_done(void *arg, int64_t tag, bool refused) {
    EstepStrands *es = arg;
    if (refused) {
        fprintf(stderr, "vanillaAlign - ERROR: the %s strand of %s does not fit the device-memory budget, left out of the expectations\n",
                es->strand, es->names[tag]);
        es->nRefused++;
    }
    if (tag == 0 && es->keepFirst) return;
    stateMachine_destruct(es->sMs[tag]);
    es->sMs[tag] = NULL;
}

static void *empty_expectations(StateMachineType type, double pseudocount, double threshold) {
    if (type == threeStateHdp) return cpecan_hdpExpectations_construct(pseudocount, threshold);
    if (type == vanilla) {
        VanillaHmmExpectations *e = calloc(1, sizeof *e);
        for (int i = 0; i < 60; i++) e->kmerSkipBins[i] = pseudocount;
        return e;
    }
    ContinuousPairHmmExpectations *e = calloc(1, sizeof *e);
    for (int i = 0; i < 9; i++) e->transitions[i] = pseudocount;
    for (int i = 0; i < NUM_OF_KMERS; i++) e->individualKmerGapProbs[i] = pseudocount;
    return e;
}

static void write_expectations(const char *path, StateMachineType type, void *e, StateMachine *first) {
    fprintf(stderr, "vanillaAlign - writing expectations to file: %s\n", path);
    FILE *fh = fopen(path, "w");
    if (!fh) die("vanillaAlign - ERROR: cannot write %s", path);
    if (type == threeStateHdp) {
        fprintf(stderr, "vanillaAlign - got %lld HDP assignments\n", (long long) ((HdpHmmExpectations *) e)->numberOfAssignments);
        cpecan_hdpExpectations_write(e, fh);
    } else if (type == vanilla) cpecan_vanillaExpectations_write(e, first, fh);
    else cpecan_pairHmmExpectations_write(e, fh);
    fclose(fh);
}

static int expectations_directory_stream(const char *dir, const char *referenceSequence, StateMachineType sMtype,
                                         const char *modelFiles[2], const char *hmmFiles[2], NanoporeHDP *nHdps[2],
                                         PairwiseAlignmentParameters *p, const cpecan_stream_options *options,
                                         const char *substitute, const char *expectationsFiles[2]) {
    int64_t n;
    char **names = read_names(dir, &n);
    cpecan_stream_options half = *options;
    if (half.deviceBytes == 0) { /* (the stream's own default, asked for here so that it can be shared out) */
        cpecan_ctx *ctx = NULL;
        const char *dev = getenv("CPECAN_DEVICE");
        if (cpecan_hip_ctx_create(dev ? atoi(dev) : 0, &ctx) != CPECAN_OK || cpecan_hip_cache_capacity(ctx, &half.deviceBytes) != CPECAN_OK)
            die("vanillaAlign - ERROR: %s", cpecan_hip_last_error());
        cpecan_hip_ctx_destroy(ctx);
    }
    half.deviceBytes /= 2;
    EstepStrands es[2];
    void *sums[2];
    cpecan_stream *streams[2];
    for (int st = 0; st < 2; st++) {
        const EstepStrands empty = { st == 0 ? "template" : "complement", names, calloc((size_t) n, sizeof(StateMachine *)),
                                     sMtype == vanilla, 0 };
        es[st] = empty;
        sums[st] = empty_expectations(sMtype, ESTEP_PSEUDOCOUNT * (double) n, p->threshold);
        streams[st] = cpecan_stream_open_expectations(p, 1, 1, &half, sums[st], estep_done, NULL, &es[st]);
    }
    for (int64_t i = 0; i < n; i++) {
        BatchRead r;
        memset(&r, 0, sizeof r);
        load_batch_read(&r, dir, names[i], referenceSequence, sMtype, p);
        for (int st = 0; st < 2; st++) {
            const NanoporeReadAdjustmentParameters npp = st == 0 ? r.npRead->templateParams : r.npRead->complementParams;
            StateMachine *sM = build_state_machine(modelFiles[st], npp, sMtype, st == 0 ? template : complement, nHdps[st]);
            if (hmmFiles[st]) hmmContinuous_loadSignalHmm(hmmFiles[st], sM, sM->type);
            char *seq = st == 0 ? r.trimmedRefSeq : r.rcTrimmedRefSeq;
            char *target = substitute ? replace_char(seq, 'C', substitute) : seq;
            Sequence *sX = sequence_construct2(sequence_correctSeqLength((int64_t) strlen(target), event), target,
                                               target_getter(sMtype), sequence_sliceNucleotideSequence2);
            stList *anchors = remapped_anchor_pairs(r.anchorPairs, st == 0 ? r.npRead->templateEventMap : r.npRead->complementEventMap,
                                                    r.pA->start2);
            es[st].sMs[i] = sM;
            cpecan_stream_submit(streams[st], i, sM, sX, r.events[st], anchors); /* (copies what it needs of the three) */
            stList_destruct(anchors);
            sequence_sequenceDestroy(sX);
            if (substitute) free(target);
        }
        r.name = NULL; /* (names[i] stays for the messages) */
        free_batch_read(&r);
    }
    int64_t nRefused = 0;
    for (int st = 0; st < 2; st++) {
        int64_t nChunks = 0, refused = 0, peak = 0;
        cpecan_stream_close(streams[st], &nChunks, &refused, &peak);
        fprintf(stderr, "vanillaAlign - %s stream: %lld chunks, at most %lld device bytes, %lld strands refused\n", es[st].strand,
                (long long) nChunks, (long long) peak, (long long) refused);
        nRefused += refused;
        write_expectations(expectationsFiles[st], sMtype, sums[st], es[st].sMs[0]);
        if (es[st].sMs[0]) stateMachine_destruct(es[st].sMs[0]);
        free(es[st].sMs);
        if (sMtype == threeStateHdp) cpecan_hdpExpectations_destruct(sums[st]);
        else free(sums[st]);
    }
    for (int64_t i = 0; i < n; i++) free(names[i]);
    free(names);
    if (nRefused == 0) fprintf(stderr, "vanillaAlign - SUCCESS: collected the expectations of %lld reads, exiting\n", (long long) n);
    return nRefused == 0 ? 0 : 1;
}

static void usage(void) {
    fprintf(stderr,
            "vanillaAlign binary, meant to be used through the signalAlign program.\n"
            "  one read:     --npRead FILE --reference FILE [--posteriors TSV | --templateExpectations T --complementExpectations C]\n"
            "                (the guide alignment, an exonerate cigar line, on stdin)\n"
            "  a directory:  --npReadDir DIR --reference FILE --outDir DIR [--stream [--streamReads N] [--streamGB X]]\n"
            "                every NAME.npRead with its NAME.cigar aligned, posteriors to outDir/NAME.tsv; --stream: in chained\n"
            "                chunks of at most N reads within X GB of device memory\n"
            "  its E-step:   --npReadDir DIR --reference FILE --stream --templateExpectations T --complementExpectations C\n"
            "                [--streamReads N] [--streamGB X] [--substitute c]\n"
            "                the expectations of all reads summed, one stream and one file per strand (half of X each); the\n"
            "                files start from the single-read pseudocount (0.0001) times the number of reads, which is what the\n"
            "                sum of the per-read files holds.  A vanilla file carries the match tables of the first read in\n"
            "                name order.\n"
            "  machines:     --strawMan, --sm3Hdp (with --templateHdp, --complementHdp), --fourState, --echelon; default vanilla\n");
}

int main(int argc, char *argv[]) {
    StateMachineType sMtype = vanilla;
    const char *npReadDir = NULL, *outDir = NULL;
    bool stream = false; /* --stream: the directory through cpecan_stream_*; --streamReads N, --streamGB X: its options */
    cpecan_stream_options streamOptions = { 0, 0, 0, 0, 0 };
    int64_t diagExpansion = 50, constraintTrim = 14;
    double threshold = 0.01;
    const char *templateModelFile = "../../cPecan/models/template_median68pA.model";
    const char *complementModelFile = "../../cPecan/models/complement_median68pA_pop2.model";
    const char *readLabel = NULL, *npReadFile = NULL, *targetFile = NULL, *posteriorProbsFile = NULL;
    const char *templateHmmFile = NULL, *complementHmmFile = NULL, *templateExpectationsFile = NULL;
    const char *complementExpectationsFile = NULL, *templateHdp = NULL, *complementHdp = NULL, *substitute = NULL;
    static struct option long_options[] = {
        { "help", no_argument, 0, 'h' }, { "strawMan", no_argument, 0, 's' }, { "sm3Hdp", no_argument, 0, 'd' },
        { "fourState", no_argument, 0, 'f' }, { "echelon", no_argument, 0, 'e' }, { "buildHDP", no_argument, 0, 'U' },
        { "HdpType", required_argument, 0, 'p' }, { "substitute", required_argument, 0, 'M' },
        { "alignments", required_argument, 0, 'a' }, { "templateModel", required_argument, 0, 'T' },
        { "complementModel", required_argument, 0, 'C' }, { "readLabel", required_argument, 0, 'L' },
        { "npRead", required_argument, 0, 'q' }, { "reference", required_argument, 0, 'r' },
        { "posteriors", required_argument, 0, 'u' }, { "inTemplateHmm", required_argument, 0, 'y' },
        { "inComplementHmm", required_argument, 0, 'z' }, { "templateHdp", required_argument, 0, 'v' },
        { "complementHdp", required_argument, 0, 'w' }, { "templateExpectations", required_argument, 0, 't' },
        { "complementExpectations", required_argument, 0, 'c' }, { "diagonalExpansion", required_argument, 0, 'x' },
        { "threshold", required_argument, 0, 'D' }, { "constraintTrim", required_argument, 0, 'm' },
        { "npReadDir", required_argument, 0, 'B' }, { "outDir", required_argument, 0, 'O' },
        { "stream", no_argument, 0, 'S' }, { "streamReads", required_argument, 0, 'R' },
        { "streamGB", required_argument, 0, 'G' }, { 0, 0, 0, 0 } };
    int key;
    while ((key = getopt_long(argc, argv, "hsdfeUp:M:a:T:C:L:q:r:u:y:z:v:w:t:c:x:D:m:B:O:SR:G:", long_options, NULL)) != -1) {
        switch (key) {
        case 's': sMtype = threeState; break;
        case 'd': sMtype = threeStateHdp; break;
        case 'f': sMtype = fourState; break;
        case 'e': sMtype = echelon; break;
        case 'U': case 'a': case 'p':
            die("vanillaAlign - building and re-sampling HDPs is outside this path (run the reference's --buildHDP)");
        case 'M': substitute = optarg; break;
        case 'T': templateModelFile = optarg; break;
        case 'C': complementModelFile = optarg; break;
        case 'L': readLabel = optarg; break;
        case 'q': npReadFile = optarg; break;
        case 'r': targetFile = optarg; break;
        case 'u': posteriorProbsFile = optarg; break;
        case 't': templateExpectationsFile = optarg; break;
        case 'c': complementExpectationsFile = optarg; break;
        case 'y': templateHmmFile = optarg; break;
        case 'z': complementHmmFile = optarg; break;
        case 'v': templateHdp = optarg; break;
        case 'w': complementHdp = optarg; break;
        case 'x': diagExpansion = atoll(optarg); break;
        case 'D': threshold = atof(optarg); break;
        case 'm': constraintTrim = atoll(optarg); break;
        case 'B': npReadDir = optarg; break;
        case 'O': outDir = optarg; break;
        case 'S': stream = true; break;
        case 'R': streamOptions.maxReadsPerChunk = atoll(optarg); break;
        case 'G': streamOptions.deviceBytes = (int64_t) (atof(optarg) * (double) (1ll << 30)); break;
        default:
            usage();
            return 1;
        }
    }
    if (sMtype == echelon && (templateExpectationsFile || complementExpectationsFile))
        die("vanillaAlign - the echelon machine has no expectations (the reference has no expectation function for it)");
    if (sMtype == echelon && (templateHmmFile || complementHmmFile))
        die("vanillaAlign - LoadSignalHmm : unupported stateMachineType (no HMM files for the echelon machine)");
    if (stream && !npReadDir) die("vanillaAlign - ERROR: --stream goes with --npReadDir and --outDir");
    if (npReadDir) { /* additive: a directory of reads as one GPU batch, or through the stream */
        const bool expectations = templateExpectationsFile || complementExpectationsFile;
        if (expectations && !stream)
            die("vanillaAlign - ERROR: --npReadDir without --stream aligns; the expectations of a directory are collected with "
                "--stream (or read by read, or by cpecan_trainModels)");
        if (expectations && !(templateExpectationsFile && complementExpectationsFile))
            die("vanillaAlign - ERROR: --templateExpectations and --complementExpectations go together");
        if (expectations && sMtype == fourState)
            die("vanillaAlign - the fourState machine has no expectations (the reference has no Hmm container for it)");
        if (!targetFile || (!outDir && !expectations)) die("vanillaAlign - ERROR: --npReadDir needs --reference and --outDir");
        if ((templateHdp != NULL) != (complementHdp != NULL)) die("Need to have template and complement HDPs");
        const char *modelFiles[2] = { templateModelFile, complementModelFile }, *hmmFiles[2] = { templateHmmFile, complementHmmFile };
        NanoporeHDP *nHdps[2] = { templateHdp ? deserialize_nhdp(templateHdp) : NULL, complementHdp ? deserialize_nhdp(complementHdp) : NULL };
        PairwiseAlignmentParameters *bp = pairwiseAlignmentBandingParameters_construct();
        bp->threshold = threshold;
        bp->constraintDiagonalTrim = constraintTrim;
        bp->diagonalExpansion = diagExpansion;
        char *reference = first_line(targetFile);
        const char *expectationsFiles[2] = { templateExpectationsFile, complementExpectationsFile };
        const int rc = expectations ? expectations_directory_stream(npReadDir, reference, sMtype, modelFiles, hmmFiles, nHdps, bp,
                                                                    &streamOptions, substitute, expectationsFiles)
                       : stream     ? align_directory_stream(npReadDir, outDir, reference, sMtype, modelFiles, hmmFiles, nHdps, bp,
                                                             &streamOptions)
                                    : align_directory(npReadDir, outDir, reference, sMtype, modelFiles, hmmFiles, nHdps, bp, substitute);
        free(reference);
        pairwiseAlignmentBandingParameters_destruct(bp);
        if (nHdps[0]) destroy_nanopore_hdp(nHdps[0]);
        if (nHdps[1]) destroy_nanopore_hdp(nHdps[1]);
        return rc;
    }
    if (!npReadFile || !targetFile) die("vanillaAlign - ERROR: --npRead and --reference are required");
    if (!readLabel) readLabel = npReadFile;
    fprintf(stderr, "vanillaAlign - using %s model\n",
            sMtype == threeState ? "strawMan" : sMtype == vanilla ? "vanilla" : sMtype == fourState ? "fourState" : sMtype == echelon ? "echelon" : "strawMan-HDP");
    if ((templateHdp != NULL) != (complementHdp != NULL)) die("Need to have template and complement HDPs");
    NanoporeHDP *nHdpT = templateHdp ? deserialize_nhdp(templateHdp) : NULL;
    NanoporeHDP *nHdpC = complementHdp ? deserialize_nhdp(complementHdp) : NULL;

    char *referenceSequence = first_line(targetFile);
    NanoporeRead *npRead = nanopore_loadNanoporeReadFromFile(npReadFile);
    if (sMtype == threeStateHdp) {
        fprintf(stderr, "vanillaAlign - descaling Nanopore Events\n");
        nanopore_descaleNanoporeRead(npRead);
    }
    PairwiseAlignmentParameters *p = pairwiseAlignmentBandingParameters_construct();
    p->threshold = threshold;
    p->constraintDiagonalTrim = constraintTrim;
    p->diagonalExpansion = diagExpansion;

    GuideAlignment *pA = cigar_read(stdin);
    char *trimmedRefSeq = pA->strand1 ? substring(referenceSequence, pA->start1, pA->end1 - pA->start1)
                                      : substring(referenceSequence, pA->end1, pA->start1 - pA->end1);
    if (!pA->strand1) {
        char *rc = reverse_complement(trimmedRefSeq);
        free(trimmedRefSeq);
        trimmedRefSeq = rc;
    }
    char *rc_trimmedRefSeq = reverse_complement(trimmedRefSeq);
    char *templateTargetSeq = substitute ? replace_char(trimmedRefSeq, 'C', substitute) : trimmedRefSeq;
    char *complementTargetSeq = substitute ? replace_char(rc_trimmedRefSeq, 'C', substitute) : rc_trimmedRefSeq;
    Sequence *tEventSequence = event_sequence_from_guide(npRead->templateEvents, pA->start2, pA->end2, npRead->templateEventMap);
    Sequence *cEventSequence = event_sequence_from_guide(npRead->complementEvents, pA->start2, pA->end2, npRead->complementEventMap);
    const int64_t rShiftT = pA->start1, rShiftC = pA->end1;
    const bool forward = pA->strand1;
    stList *anchorPairs = guide_to_anchor_pairs(pA, p);

    const bool expectations = templateExpectationsFile && complementExpectationsFile;
    if (expectations && sMtype == fourState)
        die("vanillaAlign - the fourState machine has no expectations (the reference has no Hmm container for it)");

    StrandJob jobs[2] = {
        { template, sMtype, templateModelFile, templateHmmFile, templateExpectationsFile, posteriorProbsFile, readLabel, nHdpT,
          npRead->templateParams, tEventSequence, npRead->templateEvents, npRead->templateEventMap, pA->start2,
          npRead->templateEventMap[pA->start2], rShiftT, expectations ? templateTargetSeq : trimmedRefSeq, trimmedRefSeq,
          pA->contig1, forward, p, anchorPairs, NULL, 0.0, NULL },
        { complement, sMtype, complementModelFile, complementHmmFile, complementExpectationsFile, posteriorProbsFile, readLabel,
          nHdpC, npRead->complementParams, cEventSequence, npRead->complementEvents, npRead->complementEventMap, pA->start2,
          npRead->complementEventMap[pA->start2], rShiftC, expectations ? complementTargetSeq : rc_trimmedRefSeq,
          rc_trimmedRefSeq, pA->contig1, forward, p, anchorPairs, NULL, 0.0, NULL } };
    pthread_t th[2];
    for (int i = 0; i < 2; i++) pthread_create(&th[i], NULL, expectations ? strand_expectations : strand_alignment, &jobs[i]);
    for (int i = 0; i < 2; i++) pthread_join(th[i], NULL);
    if (!expectations) {
        /* the reference's two sections append to the same file in whatever order they finish; here the rows are
         * written after both are done, template first */
        for (int i = 0; i < 2 && posteriorProbsFile; i++)
            writePosteriorProbs((char *) posteriorProbsFile, (char *) readLabel, jobs[i].sM->EMISSION_MATCH_PROBS,
                                jobs[i].npp.scale, jobs[i].npp.shift, jobs[i].allEvents, jobs[i].tsvTarget, forward,
                                pA->contig1, jobs[i].eventShift, jobs[i].referenceShift, jobs[i].alignedPairs,
                                jobs[i].strand);
        stateMachine_destruct(jobs[0].sM);
        stateMachine_destruct(jobs[1].sM);
        fprintf(stdout, "%s %lld\t%lld(%f)\t", readLabel, (long long) stList_length(anchorPairs),
                (long long) stList_length(jobs[0].alignedPairs), jobs[0].posteriorScore);
        fprintf(stdout, "%lld(%f)\n", (long long) stList_length(jobs[1].alignedPairs), jobs[1].posteriorScore);
        stList_destruct(jobs[0].alignedPairs);
        stList_destruct(jobs[1].alignedPairs);
        fprintf(stderr, "vanillaAlign - SUCCESS: finished alignment of query %s, exiting\n", readLabel);
    }
    sequence_sequenceDestroy(tEventSequence);
    sequence_sequenceDestroy(cEventSequence);
    stList_destruct(anchorPairs);
    pairwiseAlignmentBandingParameters_destruct(p);
    nanopore_nanoporeReadDestruct(npRead);
    if (nHdpT) destroy_nanopore_hdp(nHdpT);
    if (nHdpC) destroy_nanopore_hdp(nHdpC);
    return 0;
}
