// csrc_fields/fields_rule.h and csrc_fields/lzf_decode.h as a host program (tests/test_fields_core_host.py): the same text the gfx950
// kernel and librpcc_host.so are compiled from.  Every buffer is a heap block of exactly the stated size, so a sanitizer build
// (-fsanitize=address,undefined) sees any overrun.
//
//   fields_host unpack IN OUT     IN: int64 nbytes, B, total; int64 desc[B][16]; int64 row_offsets[B + 1]; the chunk's nbytes bytes.
//                                 OUT: total rows of four float32, then int32 status[B].  The loop is the kernel's without its tiles: a frame
//                                 is validated before a byte of it is read, a refused one gets +0.0 rows.
//   fields_host lzf IN OUT SIZE   IN: an LZF stream.  OUT: int32 status, int64 bytes written, then the SIZE bytes of the output block
//                                 (pre-filled with 0xA5, so that the caller sees what was left alone).
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "fields_rule.h"
#include "lzf_decode.h"

static uint8_t *slurp(const char *path, size_t *len) {
    FILE *f = fopen(path, "rb");
    if (!f || fseek(f, 0, SEEK_END)) return nullptr;
    const long n = ftell(f);
    if (n < 0 || fseek(f, 0, SEEK_SET)) return nullptr;
    uint8_t *p = (uint8_t *)malloc(n ? (size_t)n : 1);
    if (!p || fread(p, 1, (size_t)n, f) != (size_t)n) return nullptr;
    fclose(f);
    *len = (size_t)n;
    return p;
}

static int unpack(const char *in_path, const char *out_path) {
    size_t len = 0;
    uint8_t *in = slurp(in_path, &len);
    if (!in || len < 24) return 2;
    int64_t head[3];
    memcpy(head, in, 24);
    const int64_t nbytes = head[0], B = head[1], total = head[2];
    if (nbytes < 0 || B < 0 || total < 0 || len != 24 + (size_t)B * FIELDS_DESC_WORDS * 8 + (size_t)(B + 1) * 8 + (size_t)nbytes) return 2;
    int64_t *desc = (int64_t *)malloc(B ? (size_t)B * FIELDS_DESC_WORDS * 8 : 1), *offs = (int64_t *)malloc((size_t)(B + 1) * 8);
    uint8_t *chunk = (uint8_t *)malloc(nbytes ? (size_t)nbytes : 1);     // a block of its own: exactly nbytes
    uint32_t *rows = (uint32_t *)malloc(total ? (size_t)total * 16 : 1);
    int32_t *status = (int32_t *)malloc(B ? (size_t)B * 4 : 1);
    if (!desc || !offs || !chunk || !rows || !status) return 2;
    memcpy(desc, in + 24, (size_t)B * FIELDS_DESC_WORDS * 8);
    memcpy(offs, in + 24 + (size_t)B * FIELDS_DESC_WORDS * 8, (size_t)(B + 1) * 8);
    memcpy(chunk, in + len - (size_t)nbytes, (size_t)nbytes);
    free(in);
    memset(rows, 0xA5, (size_t)total * 16);
    for (int64_t b = 0; b < B; ++b) {
        const int64_t *d = desc + b * FIELDS_DESC_WORDS, r0 = offs[b], r1 = offs[b + 1];
        const bool rows_ok = r0 >= 0 && r1 >= r0 && r1 <= total;
        status[b] = rows_ok ? fields_validate(d, nbytes, r1 - r0) : FIELDS_E_LAYOUT;
        if (!rows_ok) continue;
        for (int64_t i = 0; i < r1 - r0; ++i)
            for (int c = 0; c < 4; ++c) {
                uint32_t w[2] = {0u, 0u};
                const int type = status[b] == FIELDS_OK ? (int)d[FIELDS_D_TYPE + c] : FIELDS_T_NONE;
                if (type != FIELDS_T_NONE)
                    memcpy(w, chunk + d[FIELDS_D_SPAN_OFF] + d[FIELDS_D_OFF + c] + i * d[FIELDS_D_STEP + c], (size_t)fields_size(type));
                rows[4 * (r0 + i) + c] = fields_bits(type, w[0], w[1]);
            }
    }
    FILE *g = fopen(out_path, "wb");
    if (!g || fwrite(rows, 16, (size_t)total, g) != (size_t)total || fwrite(status, 4, (size_t)B, g) != (size_t)B) return 2;
    free(desc), free(offs), free(chunk), free(rows), free(status);
    return fclose(g) ? 2 : 0;
}

static int lzf(const char *in_path, const char *out_path, const char *size_text) {
    size_t len = 0;
    uint8_t *in = slurp(in_path, &len);
    if (!in) return 2;
    const size_t size = (size_t)strtoull(size_text, nullptr, 10);
    uint8_t *src = (uint8_t *)malloc(len ? len : 1), *dst = (uint8_t *)malloc(size ? size : 1);     // exactly len and size bytes
    if (!src || !dst) return 2;
    memcpy(src, in, len);
    free(in);
    memset(dst, 0xA5, size);
    size_t got = 0;
    const int32_t rc = lzf_decode(src, len, dst, size, &got);
    const int64_t got64 = (int64_t)got;
    FILE *g = fopen(out_path, "wb");
    if (!g || fwrite(&rc, 4, 1, g) != 1 || fwrite(&got64, 8, 1, g) != 1 || fwrite(dst, 1, size, g) != size) return 2;
    free(src), free(dst);
    return fclose(g) ? 2 : 0;
}

int main(int argc, char **argv) {
    if (argc == 4 && !strcmp(argv[1], "unpack")) return unpack(argv[2], argv[3]);
    if (argc == 5 && !strcmp(argv[1], "lzf")) return lzf(argv[2], argv[3], argv[4]);
    return 2;
}
