"""The status rule of rpcc_decompress_batch (include/rpcc_hip.h) stated in NumPy, and a table of frames that break it.

A frame here is what the entropy decoders leave: the decoded bytes of its payloads (container order: salience_level, contour_map,
idx_sequence, plane_param, residual_quantized) and their statuses.  sound_frame() builds one from a seeded label map -- runs of labels along
the rows, so the contour map, the idx sequence, the model rows and the residual count fit each other as tools/decompress.py:decode_frame
asks; cases() derives the broken ones from it by named edits, each with the status the rule must give.  No GPU, no library."""
import numpy as np

KEYS = ("salience_level", "contour_map", "idx_sequence", "plane_param", "residual_quantized")
OK, E_ENTROPY, E_PLANE, E_CONTOUR, E_WIDTH, E_NSEQ, E_LABEL, E_SALIENCE, E_RESIDUAL, E_CONTAINER = range(10)


def stream_status(payload, est, P, K, uniform, levels):
    """payload: {key: decoded bytes}, est: {key: entropy status} -> the first check that fails, in decode_frame's order
    (tools/decompress.py:37-79)."""
    keys = KEYS[1:] if uniform else KEYS
    if any(est[k] != 0 for k in keys):
        return E_ENTROPY
    plane = len(payload["plane_param"])
    if plane % 16 or plane // 16 > K:
        return E_PLANE
    rows = plane // 16
    if len(payload["contour_map"]) != (P + 7) // 8:
        return E_CONTOUR
    if len(payload["idx_sequence"]) % 2 or len(payload["residual_quantized"]) % 2:
        return E_WIDTH
    idx = np.frombuffer(payload["idx_sequence"], np.uint16)
    bits = np.unpackbits(np.frombuffer(payload["contour_map"], np.uint8))[:P]
    if idx.size != int(bits.sum()):
        return E_NSEQ
    if idx.size and int(idx.max()) >= rows:
        return E_LABEL
    if not uniform:
        sal = np.frombuffer(payload["salience_level"], np.uint8)
        if sal.size > K or sal.size < rows or (sal.size and int(sal.max()) >= levels):
            return E_SALIENCE
    seg = recover_map(bits, idx)
    if len(payload["residual_quantized"]) // 2 != int((seg != 1).sum()):
        return E_RESIDUAL
    return OK


def recover_map(bits, idx):
    """Label of pixel p = idx[(contour bits at positions <= p) - 1]; 0 before the first bit."""
    k = np.cumsum(bits.astype(np.int64))
    return np.where(k > 0, np.concatenate([[0], idx.astype(np.int64)])[k], 0)


def sound_frame(H, W, K, uniform, levels, seed, rows=None):
    """A frame decode_frame accepts: labels 0 .. rows - 1 in runs of 1 .. 40 pixels (label 1, the empty pixel, among them)."""
    rng = np.random.default_rng(seed)
    P = H * W
    rows = K if rows is None else rows
    seg = np.empty(P, np.int64)
    p = 0
    while p < P:
        n = int(rng.integers(1, 41))
        seg[p: p + n] = rng.integers(0, rows)
        p += n
    seg = seg.reshape(H, W)
    contour = np.ones((H, W), bool)
    contour[:, 1:] = seg[:, 1:] != seg[:, :-1]
    payload = {"contour_map": np.packbits(contour, axis=None).tobytes(),
               "idx_sequence": seg[contour].astype(np.uint16).tobytes(),
               "plane_param": rng.normal(0, 1, (rows, 4)).astype(np.float32).tobytes(),
               "residual_quantized": rng.integers(-300, 300, int((seg != 1).sum())).astype(np.int16).tobytes()}
    payload["salience_level"] = b"" if uniform else rng.integers(0, levels, rows).astype(np.uint8).tobytes()
    return dict(name="sound_%d" % seed, payload=payload, est={k: 0 for k in KEYS}, expect=OK)


# ---- the named edits: frame -> None (in place) --------------------------------------------------------------------------------------
def _set(f, key, data):
    f["payload"][key] = bytes(data)


def entropy_refused(f, **_):
    f["est"]["residual_quantized"] = -10


def plane_truncate4(f, **_):
    _set(f, "plane_param", f["payload"]["plane_param"][:-4])


def plane_row_beyond_K(f, K, **_):
    rows = len(f["payload"]["plane_param"]) // 16
    _set(f, "plane_param", f["payload"]["plane_param"] + b"\0" * (16 * (K + 1 - rows)))


def contour_drop_byte(f, **_):
    _set(f, "contour_map", f["payload"]["contour_map"][:-1])


def residual_odd(f, **_):
    _set(f, "residual_quantized", f["payload"]["residual_quantized"] + b"\x07")


def contour_flip_bit(f, P, **_):
    a = bytearray(f["payload"]["contour_map"])
    p = P // 2 + 3          # (an in-image bit, not in the last byte)
    a[p >> 3] ^= 0x80 >> (p & 7)
    _set(f, "contour_map", a)


def contour_flip_pad_bit(f, P, **_):
    assert P % 8, "the last contour byte has pad bits only when P is no multiple of 8"
    a = bytearray(f["payload"]["contour_map"])
    a[-1] ^= 0x01
    _set(f, "contour_map", a)


def idx_equals_rows(f, **_):
    a = np.frombuffer(f["payload"]["idx_sequence"], np.uint16).copy()
    a[a.size // 3] = len(f["payload"]["plane_param"]) // 16
    _set(f, "idx_sequence", a.tobytes())


def salience_one_short(f, **_):
    _set(f, "salience_level", f["payload"]["salience_level"][: len(f["payload"]["plane_param"]) // 16 - 1])


def salience_level_equals_levels(f, levels, **_):
    a = bytearray(f["payload"]["salience_level"])
    a[len(a) // 2] = levels
    _set(f, "salience_level", a)


def residual_one_more(f, **_):
    _set(f, "residual_quantized", f["payload"]["residual_quantized"] + b"\x05\x00")


def residual_one_less(f, **_):
    _set(f, "residual_quantized", f["payload"]["residual_quantized"][:-2])


def cases(H, W, K, uniform, levels=4, seed=0):
    """[frame]: sound frames with every broken frame between them.  A broken frame = a sound frame of its own seed + the named edits, in the
    order given; `expect` is the status the rule (and the kernel) must give.  Frames with two edits trip two rules: the earlier one wins."""
    P = H * W
    table = [((entropy_refused,), E_ENTROPY), ((plane_truncate4,), E_PLANE), ((plane_row_beyond_K,), E_PLANE), ((contour_drop_byte,), E_CONTOUR),
             ((residual_odd,), E_WIDTH), ((contour_flip_bit,), E_NSEQ), ((idx_equals_rows,), E_LABEL),
             ((residual_one_more,), E_RESIDUAL), ((residual_one_less,), E_RESIDUAL),
             # two rules at once, the first in decode_frame's order wins
             ((entropy_refused, plane_truncate4), E_ENTROPY), ((contour_drop_byte, plane_truncate4), E_PLANE), ((residual_odd, contour_drop_byte), E_CONTOUR),
             ((contour_flip_bit, residual_odd), E_WIDTH), ((idx_equals_rows, contour_flip_bit), E_NSEQ), ((residual_one_more, idx_equals_rows), E_LABEL)]
    if P % 8:
        table.append(((contour_flip_pad_bit,), OK))
    if not uniform:
        table += [((salience_one_short,), E_SALIENCE), ((salience_level_equals_levels,), E_SALIENCE),
                  ((salience_level_equals_levels, idx_equals_rows), E_LABEL), ((residual_one_more, salience_level_equals_levels), E_SALIENCE)]
    out = [sound_frame(H, W, K, uniform, levels, seed)]
    for i, (edits, expect) in enumerate(table):
        # (rows below K now and then: model rows and salience entries the stream does not hold)
        f = sound_frame(H, W, K, uniform, levels, seed + 1 + i, rows=K if i % 3 else K - 2)
        for e in edits:
            e(f, P=P, K=K, levels=levels)
        f["name"], f["expect"] = "+".join(e.__name__ for e in edits), expect
        out += [f, sound_frame(H, W, K, uniform, levels, seed + 100 + i, rows=K if i % 2 else K - 3)]
    return out


def pack_batch(frames, P, K, uniform, rng):
    """The padded arrays rpcc_decompress_batch takes, every byte outside a payload 0xA5 or random: a payload longer than its row is cut at the
    row (its stated length is not).  -> dict of numpy arrays: bits u8 [B,ceil(P/8)], seq u16 [B,P], model f32 [B,K,4], q16 i16 [B,P],
    salience u8 [B,K], payload_len i64 [B,5], entropy_status i32 [B,5]."""
    B = len(frames)
    rowbytes = dict(zip(KEYS, (K, (P + 7) // 8, 2 * P, 16 * K, 2 * P)))
    raw = {}
    for j, k in enumerate(KEYS):
        a = rng.integers(0, 256, (B, rowbytes[k]), dtype=np.uint8) if j % 2 else np.full((B, rowbytes[k]), 0xA5, np.uint8)
        for b, f in enumerate(frames):
            d = np.frombuffer(f["payload"][k], np.uint8)[: rowbytes[k]]
            a[b, : d.size] = d
        raw[k] = a
    plen = np.array([[len(f["payload"][k]) for k in KEYS] for f in frames], np.int64)
    est = np.array([[f["est"][k] for k in KEYS] for f in frames], np.int32)
    if uniform:    # the salience column is ignored in the uniform framework: it may hold anything
        plen[:, 0], est[:, 0] = 123456789, -3
    return dict(bits=raw["contour_map"], seq=raw["idx_sequence"].view(np.uint16), model=raw["plane_param"].view(np.float32).reshape(B, K, 4),
                q16=raw["residual_quantized"].view(np.int16), salience=raw["salience_level"], payload_len=plen, entropy_status=est)

