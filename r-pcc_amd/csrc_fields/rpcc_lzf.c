// rpcc_lzf.c -- librpcc_host.so's LZF entry (include/rpcc_host.h): lzf_decode.h behind a C symbol.  A source of its own beside
// csrc/rpcc_host.c, so that the sources the compression library's identity is taken over (build.source_digest) do not change with it.
#include "lzf_decode.h"

int rpcc_lzf_decompress(const uint8_t *src, size_t src_bytes, uint8_t *dst, size_t dst_bytes, size_t *out_bytes) {
    static uint8_t none;
    if ((!src && src_bytes) || (!dst && dst_bytes)) return -1;
    return lzf_decode(src ? src : &none, src_bytes, dst ? dst : &none, dst_bytes, out_bytes);
}
