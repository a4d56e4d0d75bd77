/* The decoder's field walk (bd_read_ms with bd_set_umi / bd_ms_umis, include/bamdec.h) as a plain C program, to be compiled together
 * with alntools_amd/csrc/bamdec.c under -fsanitize=address,undefined and run as an executable (tests/test_collapse_umis.py).
 *
 *   bamdec_umi_smoke ok     FILE...   every file decodes; prints "FILE k <cell> <umi>" per run started (k counts a file's runs)
 *   bamdec_umi_smoke format FILE...   every file must end in BD_ERR_FORMAT from bd_read_ms, with the switch on and with it off
 * Exit status 0 and a last line "umi ok" when all of that held. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "bamdec.h"

#define BATCH 5          /* (small: a file's records come in several calls, so "the LAST call" is put to the test) */

static int read_all(const char* path, int umi_on, int print, int* n_runs) {
    bd_handle* h = NULL;
    int rc = bd_open(path, 2, &h);
    if (rc != BD_OK) { fprintf(stderr, "%s: bd_open %d\n", path, rc); return rc; }
    rc = bd_set_umi(h, umi_on);
    if (rc != BD_OK) { fprintf(stderr, "%s: bd_set_umi %d\n", path, rc); bd_close(h); return rc; }
    uint16_t flag[BATCH];
    int32_t tid[BATCH], pos[BATCH], ntid[BATCH], npos[BATCH];
    uint8_t valid[BATCH], newrun[BATCH];
    int at = 0;
    for (;;) {
        size_t n = 0, nc = 0, nu = 0;
        rc = bd_read_ms(h, BATCH, flag, tid, pos, ntid, npos, valid, newrun, &n);
        if (rc != BD_OK || n == 0) break;
        const uint8_t *cb = NULL, *ub = NULL;
        const uint32_t *co = NULL, *uo = NULL;
        rc = bd_ms_cells(h, &cb, &co, &nc);
        if (rc == BD_OK) rc = bd_ms_umis(h, &ub, &uo, &nu);
        size_t started = 0;
        for (size_t i = 0; i < n; ++i) started += newrun[i];
        if (rc != BD_OK || nc != started || nu != (umi_on ? nc : 0)) {
            fprintf(stderr, "%s: %zu runs started, %zu cells, %zu umis (rc %d)\n", path, started, nc, nu, rc);
            rc = BD_ERR_ARG;
            break;
        }
        for (size_t k = 0; k < nc; ++k, ++at)
            if (print) {
                printf("%s %d <%.*s>", path, at, (int)(co[k + 1] - co[k]), (const char*)cb + co[k]);
                if (umi_on) printf(" <%.*s>", (int)(uo[k + 1] - uo[k]), (const char*)ub + uo[k]);
                printf("\n");
            }
    }
    *n_runs = at;
    bd_close(h);
    return rc;
}

int main(int argc, char** argv) {
    if (argc < 3) { fprintf(stderr, "usage: %s ok|format FILE...\n", argv[0]); return 2; }
    const int want_format = strcmp(argv[1], "format") == 0;
    /* the argument checks */
    {
        const uint8_t* b = NULL; const uint32_t* o = NULL; size_t n = 0;
        if (bd_set_umi(NULL, 1) != BD_ERR_ARG || bd_ms_umis(NULL, &b, &o, &n) != BD_ERR_ARG) { fprintf(stderr, "a NULL handle was taken\n"); return 1; }
        bd_handle* h = NULL;
        if (bd_open(argv[2], 1, &h) != BD_OK) return 1;
        if (bd_ms_umis(h, NULL, &o, &n) != BD_ERR_ARG || bd_ms_umis(h, &b, NULL, &n) != BD_ERR_ARG || bd_ms_umis(h, &b, &o, NULL) != BD_ERR_ARG ||
            bd_ms_umis(h, &b, &o, &n) != BD_OK || n != 0 || bd_set_umi(h, 7) != BD_OK || bd_set_umi(h, 0) != BD_OK) {
            fprintf(stderr, "bd_set_umi / bd_ms_umis argument checks\n"); bd_close(h); return 1;
        }
        bd_close(h);
    }
    for (int k = 2; k < argc; ++k) {
        for (int on = 1; on >= 0; --on) {
            int n = 0;
            const int rc = read_all(argv[k], on, !want_format, &n);
            if (want_format ? rc != BD_ERR_FORMAT : rc != BD_OK) { fprintf(stderr, "%s: switch %d gave %d after %d runs\n", argv[k], on, rc, n); return 1; }
        }
    }
    printf("umi ok\n");
    return 0;
}
