/* The decoder's score walk (bd_set_score / bd_scores, include/bamdec.h) as a plain C program, to be compiled together with
 * alntools_amd/csrc/bamdec.c under -fsanitize=address,undefined and run as an executable (tests/test_best_strata.py).
 *
 *   bamdec_score_smoke ok     TAG_A TAG_B|- FILE...   every file decodes; prints "FILE i score present" per record
 *   bamdec_score_smoke format TAG_A TAG_B|- FILE...   every file must end in BD_ERR_FORMAT from bd_read, bd_read_tuples AND bd_read_ms
 * Exit status 0 and a last line "score ok" when all of that held. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bamdec.h"

#define BATCH 7          /* (small: a file's records come in several calls, so "the LAST call" is put to the test) */

static int read_all(const char* path, const char* ta, const char* tb, int how, int print, int* n_records) {
    bd_handle* h = NULL;
    int rc = bd_open(path, 2, &h);
    if (rc != BD_OK) { fprintf(stderr, "%s: bd_open %d\n", path, rc); return rc; }
    rc = bd_set_score(h, ta, tb);
    if (rc != BD_OK) { fprintf(stderr, "%s: bd_set_score %d\n", path, rc); bd_close(h); return rc; }
    uint16_t flag[BATCH];
    int32_t tid[BATCH], pos[BATCH], ntid[BATCH], npos[BATCH];
    uint8_t valid[BATCH], head[BATCH];
    uint32_t rid[BATCH], loc[BATCH], hf[BATCH], cur = 0xFFFFFFFFu;
    const int32_t n_ref = bd_n_references(h);
    uint32_t* zero = (uint32_t*)calloc((size_t)n_ref + 1, sizeof(uint32_t));
    int at = 0;
    for (;;) {
        size_t n = 0, nv = 0;
        if (how == 0) rc = bd_read(h, BATCH, 1, flag, tid, pos, ntid, npos, valid, head, &n);
        else if (how == 1) rc = bd_read_tuples(h, BATCH, 1, zero, zero, n_ref, &cur, rid, loc, hf, pos, &n, &nv);
        else rc = bd_read_ms(h, BATCH, flag, tid, pos, ntid, npos, valid, head, &n);
        if (rc != BD_OK || n == 0) break;
        const int32_t* score = NULL;
        const uint8_t* present = NULL;
        size_t ns = 0;
        rc = bd_scores(h, &score, &present, &ns);
        if (rc != BD_OK || ns != n) { fprintf(stderr, "%s: bd_scores %d, %zu scores for %zu records\n", path, rc, ns, n); rc = BD_ERR_ARG; break; }
        for (size_t i = 0; i < n; ++i, ++at)
            if (print) printf("%s %d %d %d\n", path, at, (int)score[i], (int)present[i]);
    }
    *n_records = at;
    free(zero);
    bd_close(h);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 5) { fprintf(stderr, "usage: %s ok|format TAG_A TAG_B|- FILE...\n", argv[0]); return 2; }
    const int want_format = strcmp(argv[1], "format") == 0;
    const char* ta = argv[2];
    const char* tb = strcmp(argv[3], "-") == 0 ? NULL : argv[3];
    /* the argument checks */
    if (bd_set_score(NULL, ta, tb) != BD_ERR_ARG || bd_scores(NULL, NULL, NULL, NULL) != BD_ERR_ARG) { fprintf(stderr, "a NULL handle was taken\n"); return 1; }
    for (int k = 4; k < argc; ++k) {
        for (int how = 0; how < 3; ++how) {
            int n = 0;
            const int rc = read_all(argv[k], ta, tb, how, !want_format && how == 0, &n);
            if (want_format ? rc != BD_ERR_FORMAT : rc != BD_OK) { fprintf(stderr, "%s: call kind %d gave %d after %d records\n", argv[k], how, rc, n); return 1; }
        }
    }
    /* a tag that is not two characters; a second tag without a first; off again */
    {
        bd_handle* h = NULL;
        if (bd_open(argv[4], 1, &h) != BD_OK) return 1;
        const int32_t* s = NULL; const uint8_t* p = NULL; size_t n = 99;
        if (bd_set_score(h, "A", NULL) != BD_ERR_ARG || bd_set_score(h, "AS", "YSX") != BD_ERR_ARG || bd_set_score(h, NULL, "YS") != BD_ERR_ARG ||
            bd_set_score(h, "AS", "YS") != BD_OK || bd_set_score(h, NULL, NULL) != BD_OK || bd_scores(h, &s, &p, &n) != BD_OK || n != 0) {
            fprintf(stderr, "bd_set_score's argument checks\n"); bd_close(h); return 1;
        }
        bd_close(h);
    }
    printf("score ok\n");
    return 0;
}
