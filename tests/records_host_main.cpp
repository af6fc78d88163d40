// csrc_records/records_rule.h as a host program (tests/test_records_core_host.py): the same text the gfx950 kernel is compiled from.
// Input file: records, 8 bytes each.  Output file: four float32 per record.  The buffers are heap blocks of exactly the stated sizes,
// so a sanitizer build (-fsanitize=address,undefined) sees any overrun.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "records_rule.h"

int main(int argc, char **argv) {
    if (argc != 3) return 2;
    FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
    if (!f || !g || fseek(f, 0, SEEK_END)) return 2;
    const long nbytes = ftell(f);
    if (nbytes < 0 || nbytes % RECORDS_BYTES || fseek(f, 0, SEEK_SET)) return 2;
    const size_t n = (size_t)nbytes / RECORDS_BYTES;
    uint8_t *in = (uint8_t *)malloc(n ? n * RECORDS_BYTES : 1);
    float *out = (float *)malloc(n ? n * 4 * sizeof(float) : 1);
    if (!in || !out || fread(in, RECORDS_BYTES, n, f) != n) return 2;
    for (size_t i = 0; i < n; ++i) {
        uint32_t w[2];
        memcpy(w, in + i * RECORDS_BYTES, RECORDS_BYTES);     // (little-endian host, as the device)
        records_row(w[0], w[1], out + 4 * i);
    }
    if (fwrite(out, 4 * sizeof(float), n, g) != n) return 2;
    free(in);
    free(out);
    return fclose(g) ? 2 : 0;
}
