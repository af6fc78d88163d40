// rans_filter.h -- filter 1 of the 'rans' stream format, version 2 (tests/rans_filter_ref.py is its statement in
// Python): delta of consecutive elements within a chunk, then zigzag, on elements of `width` bytes read little-endian as unsigned.
// rans_core.h includes it behind its load / store helpers.  The first part is arithmetic on one lane's own values and asks nothing new
// of the including file.  The second part, the inverse over a chunk by one wave, is compiled where the including file also defines
//   RANS_SCAN32(a)      a (uint32_t per lane) becomes its inclusive prefix sum over lanes 0 .. l, modulo 2^32
//   RANS_LAST32(a)      lane 63's a, the same value in every lane
// which rans_kernels.hip and tests/rans_filter_host_main.cpp do and tests/rans_host_main.cpp (version 1 only) does not.
#ifndef RPCC_RANS_FILTER_H
#define RPCC_RANS_FILTER_H

#define RANS_FILTER_NONE 0
#define RANS_FILTER_DELTA 1
#define RANS_UNFILTER_AHEAD 4    // blocks of 256 bytes whose dwords the inverse loads ahead

RANS_FN uint32_t rans_elem_mask(uint32_t width) { return width == 4 ? 0xFFFFFFFFu : (1u << (8 * width)) - 1u; }
RANS_FN uint32_t rans_ld_elem(const uint8_t *p, uint32_t width) { return width == 4 ? rans_ld32(p) : width == 2 ? rans_ld16(p) : p[0]; }

// z of u behind prev: d = u - prev, z = (d << 1) ^ (d >> arithmetically by all bits but the sign), all modulo 2^(8 width).
RANS_FN uint32_t rans_delta_fwd(uint32_t u, uint32_t prev, uint32_t width) {
    const uint32_t mask = rans_elem_mask(width), d = (u - prev) & mask;
    return ((d << 1) ^ (0u - (d >> (8 * width - 1)))) & mask;
}
// d of z: (z >> 1) ^ -(z & 1); the caller adds prev and masks.
RANS_FN uint32_t rans_delta_inv(uint32_t z) { return (z >> 1) ^ (0u - (z & 1u)); }

// The four filtered bytes of the dword v at a byte offset of a chunk that is a multiple of 4, all of them in whole elements; prev: the
// element in front of the dword, 0 at the chunk's start.
RANS_FN uint32_t rans_delta_dword(uint32_t v, uint32_t prev, uint32_t width) {
    if (width == 4) return rans_delta_fwd(v, prev, 4);
    const uint32_t bits = 8 * width, mask = rans_elem_mask(width);
    uint32_t out = 0;
    for (uint32_t sh = 0; sh < 32; sh += bits) {
        const uint32_t u = (v >> sh) & mask;
        out |= rans_delta_fwd(u, prev, width) << sh;
        prev = u;
    }
    return out;
}

// The filtered byte i of a chunk at src whose element is whole and not the chunk's first (width <= e, e + width <= k).  One load, the
// element and the one in front of it together (2 width bytes at src + e - width), and no condition in front of it, so that a block of
// such loads is issued together; called with a literal width.
RANS_FN uint32_t rans_delta_byte_inner(const uint8_t *src, uint32_t i, const uint32_t width) {
    const uint32_t e = i & ~(width - 1);
    uint32_t u, prev;
    if (width == 4) {
        uint64_t both;
        __builtin_memcpy(&both, src + e - 4, 8);
        prev = (uint32_t)both, u = (uint32_t)(both >> 32);
    } else {
        const uint32_t both = width == 2 ? rans_ld32(src + e - 2) : rans_ld16(src + e - 1);
        prev = both & rans_elem_mask(width), u = both >> (8 * width);
    }
    return (rans_delta_fwd(u, prev, width) >> (8 * (i - e))) & 255u;
}
// The filtered byte i of a chunk of k bytes at src, any i < k (the chunk starts at a multiple of width: chunk sizes are multiples of 4):
// the byte of its element's z -- prev = 0 for the chunk's first element -- or the byte itself where it lies behind the last whole element.
RANS_FN uint32_t rans_delta_byte(const uint8_t *src, uint32_t i, uint32_t k, uint32_t width) {
    const uint32_t e = i & ~(width - 1);
    if (e + width > k) return src[i];
    if (e == 0) return (rans_delta_fwd(rans_ld_elem(src, width), 0u, width) >> (8 * i)) & 255u;
    return width == 4 ? rans_delta_byte_inner(src, i, 4) : width == 2 ? rans_delta_byte_inner(src, i, 2) : rans_delta_byte_inner(src, i, 1);
}

#if defined(RANS_SCAN32) && defined(RANS_LAST32)
// Undoes the filter in place over the k bytes of a chunk that the same wave has just stored at out (the caller makes those stores
// visible to the wave's loads first).  Blocks of 256 bytes, four to a lane, RANS_UNFILTER_AHEAD blocks loaded at a time: a lane turns
// its own elements' z into d and sums them, one scan gives every lane the sum of the lanes before it, the carry is the last element of
// the block before.  The sums wrap modulo 2^32
// and are masked to the element when stored, so the order of the additions does not matter.  A lane stores exactly the whole elements
// it loaded; the k mod width bytes behind the last whole element are not touched.
RANS_FN void rans_unfilter_chunk(const int lane, uint8_t *out, const uint32_t k, const uint32_t width) {
    (void)lane;
    const uint32_t kw = k - (k & (width - 1)), bits = 8 * width, mask = rans_elem_mask(width), per = 4 / width;
    uint32_t carry = 0;
    for (uint32_t g0 = 0; g0 < kw; g0 += 4 * RANS_LANES * RANS_UNFILTER_AHEAD) {
        uint32_t in[RANS_NL][RANS_UNFILTER_AHEAD];
        RANS_EACH(l) {                                // all of a lane's loads first: nothing below waits for one load at a time
#pragma unroll
            for (uint32_t a = 0; a < RANS_UNFILTER_AHEAD; ++a) {
                const uint32_t at = g0 + 4 * RANS_LANES * a + 4 * (uint32_t)l;
                uint32_t w = 0;
                if (at + 4 <= kw) w = rans_ld32(out + at);
                else
                    for (uint32_t j = 0; at + j < kw && j < 4; ++j) w |= (uint32_t)out[at + j] << (8 * j);   // (beyond kw: z = 0, d = 0)
                RANS_AT(in, l)[a] = w;
            }
        }
#pragma unroll
        for (uint32_t a = 0; a < RANS_UNFILTER_AHEAD; ++a) {
            const uint32_t b0 = g0 + 4 * RANS_LANES * a;
            if (b0 >= kw) break;
            uint32_t v[RANS_NL], t[RANS_NL];
            RANS_EACH(l) {
                const uint32_t w = RANS_AT(in, l)[a];
                uint32_t s = 0, sums = 0;             // the elements' d summed within the lane, element j's sum in its place of `sums`
                for (uint32_t j = 0; j < per; ++j) {
                    s += rans_delta_inv((w >> (j * bits)) & mask);
                    sums |= (s & mask) << (j * bits);
                }
                RANS_AT(v, l) = sums, RANS_AT(t, l) = s;
            }
            RANS_SCAN32(t);
            RANS_EACH(l) {
                const uint32_t at = b0 + 4 * (uint32_t)l;
                const uint32_t own = (RANS_AT(v, l) >> ((per - 1) * bits)) & mask;   // this lane's own sum: its last element's
                const uint32_t before = carry + RANS_AT(t, l) - own;   // (t, own and carry agree modulo the element's size, which is all that is kept)
                uint32_t w = 0;
                for (uint32_t j = 0; j < per; ++j) w |= ((before + ((RANS_AT(v, l) >> (j * bits)) & mask)) & mask) << (j * bits);
                if (at + 4 <= kw) rans_st32(out + at, w);
                else
                    for (uint32_t j = 0; at + j < kw && j < 4; ++j) out[at + j] = (uint8_t)(w >> (8 * j));
            }
            carry += RANS_LAST32(t);
        }
    }
}
#endif  // RANS_SCAN32 && RANS_LAST32

#endif  // RPCC_RANS_FILTER_H
