// fields_rule.h -- the one statement of how the fields of a .pcd / .ply point record become a stored row.  Plain
// text for the host and the device: the gfx950 kernel (fields_kernels.hip) and the host program of the tests
// (tests/fields_host_main.cpp) are both compiled from it.
//
// A frame's layout is FIELDS_DESC_WORDS int64 words (include/rpcc_fields.h): span_off, span_bytes, n, off[4], step[4], type[4] for the
// columns x, y, z, w.  Element c of point i is the size(type_c) little-endian bytes at span_off + off_c + i * step_c of the chunk.
//
// The row rule, per element:
//   F32   the four bytes as they are (NaN payloads and -0.0 keep their bits)
//   F64   one round-to-nearest-even conversion to fp32; overflow gives +-inf, small values a subnormal (numpy's astype(float32))
//   I8 U8 I16 U16 I32 U32   the value converted to fp32, round-to-nearest-even (U32 16 777 217 -> 16 777 216.0)
//   NONE  +0.0
//
// fields_validate is everything the kernel checks before it reads a byte of a frame; a frame that passes names no byte outside its span
// and no span outside the chunk.
#ifndef RPCC_FIELDS_RULE_H
#define RPCC_FIELDS_RULE_H

#include <stdint.h>
#include <string.h>

#define FIELDS_DESC_WORDS 16
#define FIELDS_D_SPAN_OFF 0
#define FIELDS_D_SPAN_BYTES 1
#define FIELDS_D_N 2
#define FIELDS_D_OFF 3
#define FIELDS_D_STEP 7
#define FIELDS_D_TYPE 11
#define FIELDS_MAX_STEP 256

#define FIELDS_T_NONE 0
#define FIELDS_T_F32 1
#define FIELDS_T_F64 2
#define FIELDS_T_I8 3
#define FIELDS_T_U8 4
#define FIELDS_T_I16 5
#define FIELDS_T_U16 6
#define FIELDS_T_I32 7
#define FIELDS_T_U32 8
#define FIELDS_T_COUNT 9

#define FIELDS_OK 0
#define FIELDS_E_LAYOUT 1

// The tile rule: a workgroup stages the records of fields_tile_rows(step) points, FIELDS_STAGE_BYTES at most, and its lanes take the
// tile's points in turn (four each in a full tile of 16-byte records).
#define FIELDS_STAGE_BYTES 16384
#define FIELDS_TILE_MAX_ROWS 1024

#if defined(__HIPCC__)
#define FIELDS_HD __host__ __device__ __forceinline__
#else
#define FIELDS_HD static inline
#endif

FIELDS_HD int fields_size(int64_t type) {
    switch (type) {
        case FIELDS_T_F64: return 8;
        case FIELDS_T_F32: case FIELDS_T_I32: case FIELDS_T_U32: return 4;
        case FIELDS_T_I16: case FIELDS_T_U16: return 2;
        case FIELDS_T_I8: case FIELDS_T_U8: return 1;
        default: return 0;
    }
}

FIELDS_HD uint32_t fields_float_bits(float f) {
    uint32_t u;
    memcpy(&u, &f, 4);
    return u;
}

// The fp32 bits of one element.  lo: its first four bytes, little endian (bytes past the element's size are ignored); hi: bytes 4 .. 7
// (read for F64 only).
FIELDS_HD uint32_t fields_bits(int type, uint32_t lo, uint32_t hi) {
    switch (type) {
        case FIELDS_T_F32: return lo;
        case FIELDS_T_F64: {
            const uint64_t u = (uint64_t)hi << 32 | lo;
            double d;
            memcpy(&d, &u, 8);
            return fields_float_bits((float)d);
        }
        case FIELDS_T_I8: return fields_float_bits((float)(int32_t)(int8_t)(lo & 0xffu));
        case FIELDS_T_U8: return fields_float_bits((float)(lo & 0xffu));
        case FIELDS_T_I16: return fields_float_bits((float)(int32_t)(int16_t)(lo & 0xffffu));
        case FIELDS_T_U16: return fields_float_bits((float)(lo & 0xffffu));
        case FIELDS_T_I32: return fields_float_bits((float)(int32_t)lo);
        case FIELDS_T_U32: return fields_float_bits((float)lo);
        default: return 0u;   // NONE: +0.0
    }
}

// Points of one tile for a frame whose largest step is max_step (1 .. FIELDS_MAX_STEP): 1024 up to a step of 16, 512 at 32, 64 at 256.
FIELDS_HD int fields_tile_rows(int64_t max_step) {
    const int64_t r = FIELDS_STAGE_BYTES / max_step;
    return (int)(r < FIELDS_TILE_MAX_ROWS ? r : FIELDS_TILE_MAX_ROWS);
}

// The largest step of the frame's present columns (a validated descriptor).
FIELDS_HD int64_t fields_max_step(const int64_t *d) {
    int64_t m = 1;
    for (int c = 0; c < 4; ++c)
        if (d[FIELDS_D_TYPE + c] != FIELDS_T_NONE && d[FIELDS_D_STEP + c] > m) m = d[FIELDS_D_STEP + c];
    return m;
}

// d: the frame's descriptor; nbytes: the chunk; rows: row_offsets[b+1] - row_offsets[b].  FIELDS_OK, or FIELDS_E_LAYOUT.  No product
// below can overflow: n <= 2^31 and step <= 256 when they are multiplied.
FIELDS_HD int fields_validate(const int64_t *d, int64_t nbytes, int64_t rows) {
    const int64_t span_off = d[FIELDS_D_SPAN_OFF], span_bytes = d[FIELDS_D_SPAN_BYTES], n = d[FIELDS_D_N];
    if (span_off < 0 || span_bytes < 0 || span_off > nbytes || span_bytes > nbytes - span_off) return FIELDS_E_LAYOUT;
    if (n < 0 || n > 2147483647 || n != rows) return FIELDS_E_LAYOUT;
    for (int c = 0; c < 4; ++c) {
        const int64_t type = d[FIELDS_D_TYPE + c], off = d[FIELDS_D_OFF + c], step = d[FIELDS_D_STEP + c];
        if (type < 0 || type >= FIELDS_T_COUNT) return FIELDS_E_LAYOUT;
        if (type == FIELDS_T_NONE) {
            if (c < 3) return FIELDS_E_LAYOUT;   // x, y and z are needed
            continue;
        }
        const int64_t size = fields_size(type);
        if (step < size || step > FIELDS_MAX_STEP) return FIELDS_E_LAYOUT;
        if (n > 0) {
            if (off < 0 || off > span_bytes || size > span_bytes - off) return FIELDS_E_LAYOUT;
            if ((n - 1) * step > span_bytes - off - size) return FIELDS_E_LAYOUT;
        }
    }
    return FIELDS_OK;
}

#endif  // RPCC_FIELDS_RULE_H
