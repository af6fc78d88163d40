/* beam_index.h -- the per-beam elevation index of rpcc_project_beams (include/rpcc_hip.h), built on the host.
 * Plain C (also compiled as C++): no device call, no allocation, nothing but the caller's two arrays is touched.  The same text is
 * built into librpcc_hip.so (rpcc_beam_index_build) and into tests/beam_index_host_main.cpp (address / undefined-behaviour sanitizers).
 *
 * Layout of the index for H beams, RPCC_BEAM_INDEX_BYTES(H) = 24 H bytes, 8-byte aligned:
 *   f64 va[H]      the table in row order (row h of the image = entry h): what the exact sequence's arg-min walks
 *   f64 sorted[H]  the table ascending (stable: equal entries keep their row order)
 *   f32 mid[H]     mid[k] = (float)((sorted[k] + sorted[k + 1]) / 2) for k < H - 1; mid[H - 1] = +inf (pad)
 *   i32 row[H]     sorted position -> row; every member of a run of equal entries maps to the run's lowest row (the reference's
 *                  first-minimum arg-min never returns another)                                                                   */
#ifndef RPCC_BEAM_INDEX_H
#define RPCC_BEAM_INDEX_H

#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifndef RPCC_BEAM_MAX_H
#define RPCC_BEAM_MAX_H 128
#endif
#define RPCC_BEAM_INDEX_BYTES(H) ((size_t)24 * (size_t)(H))

/* 0 = built; -1 = H outside 1 .. RPCC_BEAM_MAX_H, a NULL pointer or a table entry that is NaN or +-inf (out is then untouched). */
static inline int rpcc_beam_index_build_impl(const double *angles, int H, void *out) {
    if (angles == NULL || out == NULL || H < 1 || H > RPCC_BEAM_MAX_H) return -1;
    for (int h = 0; h < H; h++)
        if (!(fabs(angles[h]) <= 1.7976931348623157e308)) return -1;
    double sorted[RPCC_BEAM_MAX_H];
    float mid[RPCC_BEAM_MAX_H];
    int32_t row[RPCC_BEAM_MAX_H];
    for (int h = 0; h < H; h++) {   /* insertion sort, stable: an entry moves past strictly larger ones only */
        const double v = angles[h];
        int k = h;
        while (k > 0 && sorted[k - 1] > v) { sorted[k] = sorted[k - 1]; row[k] = row[k - 1]; k--; }
        sorted[k] = v; row[k] = h;
    }
    for (int k = 1; k < H; k++)
        if (sorted[k] == sorted[k - 1]) row[k] = row[k - 1];   /* (rows ascend inside a run: the first is the lowest) */
    for (int k = 0; k + 1 < H; k++) mid[k] = (float)(sorted[k] * 0.5 + sorted[k + 1] * 0.5);   /* (halves first: no overflow) */
    mid[H - 1] = INFINITY;
    char *o = (char *)out;
    memcpy(o, angles, (size_t)H * 8);
    memcpy(o + (size_t)H * 8, sorted, (size_t)H * 8);
    memcpy(o + (size_t)H * 16, mid, (size_t)H * 4);
    memcpy(o + (size_t)H * 20, row, (size_t)H * 4);
    return 0;
}

#endif
