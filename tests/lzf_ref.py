"""The liblzf stream format of a .pcd file's `DATA binary_compressed` body in slow pure Python: the decoder r-pcc_amd/csrc_fields/lzf_decode.h
states in C, and a greedy encoder, for making fixtures (tests/pointfile_cases.py) and for holding the C decoder to (tests/test_pointfile.py).

A control byte c < 32 is followed by c + 1 literals.  Otherwise len = c >> 5, grown by the next byte when it is 7; the distance is
((c & 31) << 8 | next byte) + 1; len + 2 bytes are copied from `distance` back, one byte at a time."""

OK, E_TRUNCATED, E_DISTANCE, E_OVERFLOW = 0, 1, 2, 3
MAX_LITERALS = 32
MIN_MATCH, MAX_MATCH = 3, 2 + 7 + 255
MAX_DISTANCE = 1 << 13


def literals(data):
    """The literal runs that spell `data`."""
    out = bytearray()
    for lo in range(0, len(data), MAX_LITERALS):
        run = data[lo: lo + MAX_LITERALS]
        out.append(len(run) - 1)
        out += run
    return bytes(out)


def match(length, distance):
    """One match of `length` bytes (3 .. 264) from `distance` (1 .. 8192) back."""
    assert MIN_MATCH <= length <= MAX_MATCH and 1 <= distance <= MAX_DISTANCE
    l, d = length - 2, distance - 1
    if l < 7:
        return bytes([l << 5 | d >> 8, d & 255])
    return bytes([7 << 5 | d >> 8, l - 7, d & 255])


def decode(src, dst_bytes):
    """-> (status, the bytes written before it): the decoder of lzf_decode.h, statement by statement."""
    src = bytes(src)
    out = bytearray()
    ip = 0
    while ip < len(src):
        c = src[ip]
        ip += 1
        if c < 32:
            run = c + 1
            if run > len(src) - ip:
                return E_TRUNCATED, bytes(out)
            if run > dst_bytes - len(out):
                return E_OVERFLOW, bytes(out)
            out += src[ip: ip + run]
            ip += run
        else:
            length = c >> 5
            if length == 7:
                if ip >= len(src):
                    return E_TRUNCATED, bytes(out)
                length += src[ip]
                ip += 1
            if ip >= len(src):
                return E_TRUNCATED, bytes(out)
            distance = ((c & 31) << 8 | src[ip]) + 1
            ip += 1
            length += 2
            if distance > len(out):
                return E_DISTANCE, bytes(out)
            if length > dst_bytes - len(out):
                return E_OVERFLOW, bytes(out)
            for _ in range(length):
                out.append(out[-distance])
    return OK, bytes(out)


def encode(data):
    """A greedy encoder: at every position the longest match of the most recent 16 candidates that share its first three bytes."""
    data = bytes(data)
    out, pending = bytearray(), bytearray()
    seen = {}
    i = 0

    def note(k):
        if k + MIN_MATCH <= len(data):
            seen.setdefault(data[k: k + MIN_MATCH], []).append(k)

    while i < len(data):
        best_len, best_dist = 0, 0
        for j in reversed(seen.get(data[i: i + MIN_MATCH], [])[-16:]):
            if i - j > MAX_DISTANCE:
                break
            k = 0
            while k < MAX_MATCH and i + k < len(data) and data[j + k] == data[i + k]:
                k += 1
            if k > best_len:
                best_len, best_dist = k, i - j
        if best_len >= MIN_MATCH:
            out += literals(bytes(pending))
            pending.clear()
            out += match(best_len, best_dist)
            for k in range(i, i + best_len):
                note(k)
            i += best_len
        else:
            pending.append(data[i])
            note(i)
            i += 1
    out += literals(bytes(pending))
    return bytes(out)
