/* The caller-record table (include/trx.h, "CALLER RECORDS") walked through the oracle's orc_ao_ray_inst, for a build with
 * -fsanitize=address,undefined (tests/test_caller_records.py compiles this file together with oracle/trx_oracle.c and runs
 * it as a child process).  The triangle table and the instance rows are heap blocks of exactly n_tris * 9 and
 * n_instances * 12 floats: a read formed from an id outside them is a heap-buffer-overflow report, a wrong answer a
 * non-zero exit.  The expected answers are the columns written out below, not a second evaluation of the rule. */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "trx_oracle.h"

#define N_TRIS 5u
#define N_INST 3u

static float bits(uint32_t u) {
    float f;
    memcpy(&f, &u, 4);
    return f;
}

int main(void) {
    /* t, and whether it is below FLT_MAX (the pixel's "own" t of the Python table is the 2.5 here) */
    const float ts[8] = {2.5f, 1.0f, -1.0f, 0.0f, bits(0x7F7FFFFEu), bits(0x7F7FFFFFu), INFINITY, NAN};
    const int t_ok[8] = {1, 1, 1, 1, 1, 0, 0, 0};
    /* prim, and whether it is inside a table of N_TRIS triangles */
    const uint32_t prims[9] = {0u, N_TRIS - 1u, N_TRIS, N_TRIS + 1u, 0x80000000u, 0x55555556u, 0xAAAAAAABu, 0xFFFFFFFEu, 0xFFFFFFFFu};
    const int p_ok[9] = {1, 1, 0, 0, 0, 0, 0, 0, 0};
    /* instance id, and whether it selects one of N_INST rows */
    const uint32_t insts[7] = {0u, N_INST - 1u, N_INST, N_INST + 1u, 0x80000000u, 0xFFFFFFFEu, 0xFFFFFFFFu};
    const int i_ok[7] = {1, 1, 0, 0, 0, 0, 0};

    float *tris = malloc(sizeof(float) * 9 * N_TRIS);
    float *rows = malloc(sizeof(float) * 12 * N_INST);
    if (!tris || !rows) return 2;
    for (uint32_t k = 0; k < N_TRIS; k++) { /* {v0, e1, e2} with a normal that differs per triangle */
        const float tri[9] = {0.f, 0.f, -3.f - (float)k, 1.f, 0.25f * (float)k, 0.f, 0.f, 1.f, 0.125f * (float)k};
        memcpy(tris + 9 * k, tri, sizeof(tri));
    }
    for (uint32_t k = 0; k < N_INST; k++) { /* a scale and a shear per instance, so a row changes the normal */
        const float row[12] = {1.f + (float)k, 0.5f, 0.f, 0.25f, 0.f, 2.f, 0.f, -1.f, 0.25f * (float)k, 0.f, 0.5f, 3.f};
        memcpy(rows + 12 * k, row, sizeof(row));
    }
    orc_view view;
    const float eye[3] = {0.f, 0.f, 2.f}, look[3] = {0.f, 0.f, 0.f};
    orc_view_from_camera(eye, look, 60.0f, 16.0f, 8.0f, &view);

    int bad = 0, calls = 0;
    for (int with_rows = 0; with_rows < 2; with_rows++) {
        orc_scene s;
        memset(&s, 0, sizeof(s));
        s.tris = tris;
        s.n_tris = N_TRIS;
        s.n_instances = N_INST;
        s.instance_w2o = with_rows ? rows : NULL;
        for (int a = 0; a < 8; a++)
            for (int b = 0; b < 9; b++)
                for (int c = 0; c < 7; c++) {
                    const orc_hit h = {ts[a], prims[b]};
                    float o[3] = {0.f, 0.f, 0.f}, d[3] = {0.f, 0.f, 0.f};
                    const int got = orc_ao_ray_inst(&s, &view, 16, 8, (uint32_t)(a + c) % 16u, (uint32_t)b % 8u, h, insts[c], 7u, 0.01f, o, d);
                    const int want = t_ok[a] && p_ok[b];
                    calls++;
                    if (got != want) {
                        printf("t %d prim 0x%08x inst 0x%08x rows %d: returned %d, the rule says %d\n", a, prims[b], insts[c], with_rows, got, want);
                        bad++;
                        continue;
                    }
                    if (!want) continue;
                    /* the direction is that of the same triangle under the same row - no row where the id selects none */
                    const orc_hit plain = {1.0f, prims[b]};
                    float o2[3], d2[3];
                    if (!orc_ao_ray_inst(&s, &view, 16, 8, (uint32_t)(a + c) % 16u, (uint32_t)b % 8u, plain, i_ok[c] ? insts[c] : 0xFFFFFFFFu, 7u,
                                         0.01f, o2, d2) ||
                        memcmp(d, d2, sizeof(d)) != 0) {
                        printf("t %d prim 0x%08x inst 0x%08x rows %d: the direction is not the %s's\n", a, prims[b], insts[c], with_rows,
                               i_ok[c] ? "row" : "object-space normal");
                        bad++;
                    }
                }
    }
    free(tris);
    free(rows);
    printf("caller records: %d calls, %d wrong\n", calls, bad);
    return bad ? 1 : 0;
}
