// records_rule.h -- the one statement of how an NCLT velodyne_sync record becomes a stored row.  Plain text
// for the host and the device: the gfx950 kernel (records_kernels.hip) and the host program of the tests (tests/records_host_main.cpp)
// are both compiled from it.
//
// A record is 8 bytes, little endian, no header:  <H x_s, <H y_s, <H z_s, B intensity, B laser.  As two 32-bit words:
//   w0 = x_s | y_s << 16,   w1 = z_s | intensity << 16 | laser << 24.
// A coordinate is  (float)((double)v_s * 0.005 + (-100.0)):  the fp64 product rounded, the fp64 sum rounded, one rounding to fp32 --
// what the reference computes in Python floats (dataset/datasets/nclt_dataset.py:57-63) and then stores with .astype(np.float32)
// (:32-33).  The fourth float of the row is the intensity byte (exact); the reference writes 0 there and never reads it.  The laser
// byte is not read.
//
// The product and the sum must stay two roundings.  A fused multiply-add changes the fp32 result at exactly one of the 65 536 field
// values, v_s = 20000: the sensor origin, where the rule gives +0.0 and the FMA a tiny non-zero number that passes the projection's
// zero-range test.  The libraries are built with -ffp-contract=off; the function below also says so itself.
#ifndef RPCC_RECORDS_RULE_H
#define RPCC_RECORDS_RULE_H

#include <stdint.h>

#define RECORDS_BYTES 8
#define RECORDS_SCALING 0.005   // 5 mm
#define RECORDS_OFFSET (-100.0)

#if defined(__HIPCC__)
#define RECORDS_HD __host__ __device__ __forceinline__
#else
#define RECORDS_HD static inline
#endif

// No contraction inside records_coord, whatever the command line says: clang (hipcc, host and device) takes the pragma at the head of
// the body, gcc the function attribute.
#if defined(__clang__)
#define RECORDS_UNFUSED_FN
#define RECORDS_UNFUSED_BODY _Pragma("clang fp contract(off)")
#elif defined(__GNUC__)
#define RECORDS_UNFUSED_FN __attribute__((optimize("fp-contract=off")))
#define RECORDS_UNFUSED_BODY
#else
#define RECORDS_UNFUSED_FN
#define RECORDS_UNFUSED_BODY
#endif

RECORDS_UNFUSED_FN RECORDS_HD float records_coord(uint32_t v_s) {
    RECORDS_UNFUSED_BODY
    const double scaled = (double)v_s * RECORDS_SCALING;   // rounded here ...
    const double v = scaled + RECORDS_OFFSET;              // ... and here
    return (float)v;
}

RECORDS_HD uint32_t records_x(uint32_t w0) { return w0 & 0xffffu; }
RECORDS_HD uint32_t records_y(uint32_t w0) { return w0 >> 16; }
RECORDS_HD uint32_t records_z(uint32_t w1) { return w1 & 0xffffu; }
RECORDS_HD float records_intensity(uint32_t w1) { return (float)((w1 >> 16) & 0xffu); }

// The row (x, y, z, intensity) of the record (w0, w1).
RECORDS_HD void records_row(uint32_t w0, uint32_t w1, float row[4]) {
    row[0] = records_coord(records_x(w0));
    row[1] = records_coord(records_y(w0));
    row[2] = records_coord(records_z(w1));
    row[3] = records_intensity(w1);
}

#endif  // RPCC_RECORDS_RULE_H
