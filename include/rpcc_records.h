/*
 * rpcc_records.h -- C ABI of librpcc_records.so: NCLT velodyne_sync records unpacked to stored rows on the MI355X (gfx950), the
 * device counterpart of the reference's NcltDataset.load_original_utf8_data / convert and the cast of its
 * preprocess_original_utf8_to_bin_file (dataset/datasets/nclt_dataset.py:13-63).  A library of its own, apart from librpcc_hip.so.
 *
 * Conventions as in rpcc_filter.h: plain pointers and sizes; every pointer marked "dev" is a device pointer; the kernel is enqueued
 * on the caller's hipStream_t (passed as void*) and nothing synchronises; the library allocates nothing and takes no work buffer;
 * 0 = OK, negative = error with the text in rpcc_records_last_error().  Argument errors return RPCC_RECORDS_ERR_ARG before anything
 * touches the device.
 *
 * A record is 8 bytes, little endian, no header: uint16 x_s, y_s, z_s, uint8 intensity, uint8 laser.  Its row is four float32:
 * (float)((double)v_s * 0.005 + (-100.0)) for x, y, z -- two fp64 roundings, un-fused, then one to fp32 -- and the intensity byte
 * as a float.  The laser byte is not read.  DESIGN.md section 21 states the whole specification.
 */
#ifndef RPCC_RECORDS_H
#define RPCC_RECORDS_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RPCC_RECORDS_ABI_VERSION 1
#define RPCC_RECORDS_ERR_ARG (-1)
#define RPCC_RECORDS_ERR_HIP (-2)
#define RPCC_RECORDS_BYTES 8                 /* bytes of a record */
#define RPCC_RECORDS_MAX_TOTAL 2147483647    /* records per call: what the batch calls take as `total` */

int rpcc_records_version(void);
const char *rpcc_records_last_error(void);

/* Unpacks `total` records.  records (dev): total * 8 bytes, 8-byte aligned (16-byte alignment is not needed: a buffer that starts one
 * record into an aligned allocation is served at the same rate).  rows (dev, f32 [total,4]): 16-byte aligned; the stored-row layout every
 * entry of librpcc_hip.so reads with point_stride_bytes = 16.  0 <= total <= RPCC_RECORDS_MAX_TOTAL; with total == 0 nothing is launched
 * and both pointers may be NULL.  The two buffers must not overlap.  rows is written completely -- it may hold anything before -- and
 * nothing outside its total * 16 bytes is touched; the result repeats bit for bit. */
int rpcc_records_unpack(const void *records, int64_t total, float *rows, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* RPCC_RECORDS_H */
