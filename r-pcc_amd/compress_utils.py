"""Mirror of the reference's utils/compress_utils.py: QuantizationModule on the HIP path, payload
packing, the .rpcc container and the entropy back-ends (stdlib calls, excluded from the measured path).

basic_compressor 'rans' is not one of the reference's methods: it is the build's own chunk-parallel rANS format (rpcc_amd.rans_codec,
DESIGN.md section 19), coded and read on the GPU only -- there is no host coder, the reference project cannot read such containers and
neither can a machine without a GPU.
"""
import bz2
import collections
import copy
import gzip
import importlib
import os
import struct

import numpy as np
import torch

from . import ops
from .contour_utils import ContourExtractor
from .utils import load_yaml


def _dev(a, device, dtype=None):
    a = np.ascontiguousarray(a)
    if dtype is not None:
        a = a.astype(dtype)
    return torch.from_numpy(a).to(device)


class QuantizationModule:
    """utils/compress_utils.py:35-132."""

    def __init__(self, base_accuracy, level_kp_num=(30, 10, 3, 0), level_dacc=(0, 0.02, 0.04, 0.06),
                 ground_salience_level=2, feature_region=3, segments=8, sharp_num=4, less_sharp_num=8, flat_num=6,
                 uniform=True, device="cuda:0"):
        self.uniform = uniform
        self.device = torch.device(device)
        if uniform:
            self.acc = base_accuracy
        else:
            self.level_kp_num = np.array(level_kp_num)
            self.acc = np.array([base_accuracy] * len(self.level_kp_num)) + np.array(level_dacc)
            self.ground_level = ground_salience_level
            self.feature_region = feature_region
            self.segments = segments
            self.sharp_num = sharp_num
            self.less_sharp_num = less_sharp_num
            self.flat_num = flat_num

    def quantize_residual(self, residual, seg_idx, point_cloud=None, range_image=None):
        """-> (residual_quantized int32 [nnz], salience_level int32 [max+1] or None, key_point_map or None)."""
        h, w = seg_idx.shape[:2]
        M = max(int(seg_idx.max()) - 1, 1)
        K = M + 2
        # the stage entries exist for uint16 labels too (rpcc_predict_quantize_wide, rpcc_extract_features_wide, rpcc_salience_wide: cluster_num <= 1022;
        # the batch front-end, pipeline.BatchCompressor, goes up to 65533)
        ops.check_cluster_num(M, stage="mid")
        seg = _dev(seg_idx, self.device, np.uint16 if ops.is_wide(M) else np.uint8).reshape(1, h, w)
        res = _dev(residual, self.device, np.float32).reshape(1, h * w)
        dummy_model = torch.zeros((1, K, 4), dtype=torch.float32, device=self.device)
        tm = torch.zeros((h * w, 3), dtype=torch.float32, device=self.device)
        ri0 = torch.zeros((1, h, w), dtype=torch.float32, device=self.device)
        if self.uniform:
            q, nnz, _ = ops.predict_quantize(ri0, tm, seg, dummy_model, self.acc, M, residual=res)
            return q[0, : int(nnz[0])].cpu().numpy(), None, None
        ri = _dev(range_image, self.device, np.float32).reshape(1, h, w)
        _, kp = ops.extract_features(ri, seg, self.feature_region, self.segments, self.sharp_num, self.less_sharp_num,
                                     self.flat_num)
        sal, label_acc = ops.salience(seg, kp, self.level_kp_num, self.acc.astype(np.float32), self.ground_level, M)
        q, nnz, _ = ops.predict_quantize(ri0, tm, seg, dummy_model, 0.0, M, residual=res, label_acc=label_acc)
        nrow = int(seg_idx.max()) + 1
        return (q[0, : int(nnz[0])].cpu().numpy(), sal[0, :nrow].cpu().numpy().astype(np.int32),
                kp[0].cpu().numpy().astype(np.int32))

    def dequantize_residual(self, quantized_residual, seg_idx, salience_level=None):
        """utils/compress_utils.py:114-132 -> f32 [H,W,1] (decoder; on the device via rpcc_decode with a
        zero model, so pred = 0 and rec = residual; labels above 255: uint16 through rpcc_decode_wide)."""
        h, w = seg_idx.shape[:2]
        M = max(int(seg_idx.max()) - 1, 1)
        seg = _dev(seg_idx, self.device, np.uint16 if ops.is_wide(M) else np.uint8).reshape(1, h, w)
        K = M + 2
        q = torch.zeros((1, h * w), dtype=torch.int16, device=self.device)
        qq = _dev(quantized_residual, self.device, np.int16)
        q[0, : qq.numel()] = qq
        model = torch.zeros((1, K, 4), dtype=torch.float32, device=self.device)
        tm = torch.zeros((h * w, 3), dtype=torch.float32, device=self.device)
        if self.uniform:
            rec, _ = ops.decode(seg, q, model, tm, self.acc)
        else:
            sal = torch.zeros((1, K), dtype=torch.uint8, device=self.device)
            s = _dev(salience_level, self.device, np.uint8)
            sal[0, : s.numel()] = s
            rec, _ = ops.decode(seg, q, model, tm, list(self.acc), salience=sal)
        return np.expand_dims(rec[0].cpu().numpy(), -1)


def compress_point_cloud(basic_compressor, plane_param, cluster_idx, salience_level, nonzero_residual_quantized,
                         ground_residual_quantized=None, cluster_residual_quantized=None, point_cloud=None,
                         range_image=None, full=False, intensity=None, subpixel=None, hidden_points=None):
    """utils/compress_utils.py:138-164: casts + contour + packbits + per-array entropy coding.  intensity (not the reference's): the
    uint8 payload of ops.intensity_encode, coded like any other array and appended to the container by pack_bitstream.  subpixel: the
    uint8 payload of ops.subpixel_encode, alike, behind it.  hidden_points: the uint8 payload of ops.hidden_encode, alike, last."""
    original_data = {"residual_quantized": np.asarray(nonzero_residual_quantized).astype(np.int16)}
    if intensity is not None:
        original_data["intensity"] = np.ascontiguousarray(intensity, dtype=np.uint8)
    if subpixel is not None:
        original_data["subpixel"] = np.ascontiguousarray(subpixel, dtype=np.uint8)
    if hidden_points is not None:
        original_data["hidden_points"] = np.ascontiguousarray(hidden_points, dtype=np.uint8)
    if full:
        if point_cloud is not None:
            original_data["point_cloud"] = point_cloud.astype(np.float32)
        if range_image is not None:
            original_data["range_image"] = range_image.astype(np.float32)
        if ground_residual_quantized is not None:
            original_data["ground_residual"] = ground_residual_quantized.astype(np.int16)
        if cluster_residual_quantized is not None:
            original_data["cluster_residual"] = cluster_residual_quantized.astype(np.int16)
    if salience_level is not None:
        original_data["salience_level"] = np.asarray(salience_level).astype(np.uint8)
    contour_map, idx_sequence = ContourExtractor.extract_contour(cluster_idx)
    original_data["contour_map"] = np.packbits(contour_map.astype(bool), axis=None).astype(np.uint8)
    original_data["idx_sequence"] = idx_sequence.astype(np.uint16)
    original_data["plane_param"] = np.asarray(plane_param).astype(np.float32)
    return original_data, basic_compressor.compress_dict(original_data)


# The .rpcc container's payloads, one row each, in file order: the name, the dtype of the decoded array, the decoded bytes of one frame at
# most as a function of (P pixels, K = cluster_num + 2 model rows), and the per-frame count that cuts the frame's part out of the batch's
# buffer (frame_slices).  Everything else that is said about a column is derived from its row: the element width handed to rANS is
# dtype.itemsize, the delta filter is rans_codec.delta_filter(dtype).
Column = collections.namedtuple("Column", "name dtype bound cut")
SCHEMA = (Column("salience_level", np.dtype(np.uint8), lambda P, K: K, "nrow"),
          Column("contour_map", np.dtype(np.uint8), lambda P, K: (P + 7) // 8, "row"),
          Column("idx_sequence", np.dtype(np.uint16), lambda P, K: 2 * P, "nseq"),
          Column("plane_param", np.dtype(np.float32), lambda P, K: 16 * K, "nrow"),
          Column("residual_quantized", np.dtype(np.int16), lambda P, K: 2 * P, "nnz"),
          Column("intensity", np.dtype(np.uint8), lambda P, K: 8 + P, "nbytes"),
          Column("subpixel", np.dtype(np.uint8), lambda P, K: 8 + 2 * P, "nsub"))
# The hidden_points column stands beside SCHEMA: its bound needs the frame's point count N besides P (16 + P + 4 N)
HIDDEN_COLUMN = Column("hidden_points", np.dtype(np.uint8), lambda P, K, N=0: 16 + P + 4 * N, "nhid")
INTENSITY_MAGIC = b"RPI1"
SUBPIXEL_MAGIC = b"RPS1"
HIDDEN_MAGIC = b"RPH1"
TRAILERS = ("intensity", "subpixel", "hidden_points")      # the optional columns behind the geometry, in file order


def columns(uniform, intensity=False, subpixel=False, hidden_points=False):
    """The rows of SCHEMA a container holds, in file order: salience first with the non-uniform framework, then the trailers no
    reference reader looks at, where they are carried: intensity, then subpixel, then hidden_points (HIDDEN_COLUMN)."""
    return SCHEMA[1 if uniform else 0: 5] + tuple(c for c, on in zip(SCHEMA[5:] + (HIDDEN_COLUMN,), (intensity, subpixel, hidden_points)) if on)


def _keys(uniform, data=()):
    """The arrays of a container in file order; 'intensity', 'subpixel' and 'hidden_points' where the frame holds them."""
    return tuple(c.name for c in columns(uniform, "intensity" in data, "subpixel" in data, "hidden_points" in data))


def payload_spans(blob, count):
    """The one walk over a container: [int32 length | bytes] per payload.  Yields (start, length) of the first count payloads and ends
    before the first one the blob does not hold: a prefix that is cut off or negative, or a payload longer than the bytes left."""
    off = 0
    for _ in range(count):
        if off + 4 > len(blob):
            return
        (n,) = struct.unpack_from("i", blob, off)
        if n < 0 or off + 4 + n > len(blob):
            return
        yield off + 4, n
        off += 4 + n


def frame_slices(cols, buffers, counts, nnz, nseq, nbytes=None, nsub=None, nhid=None):
    """Which elements of which buffer are frame b's column c, stated once for the host assembly (BatchPayload: arrays read back or pinned)
    and for the device containers (addresses).  buffers: {column name: the batch's buffer}; counts [B,K], nnz / nseq / nbytes / nsub [B] -- all
    numpy arrays or all torch tensors of one device.  -> {name: (start, length)}, int64 [B] of the same kind, in elements of the column's
    dtype into the flattened buffer.  By the column's cut: 'row', 'nrow', 'nbytes' and 'nsub' columns are rows of a padded [B, ...] array -- the
    whole row, its first nrow sub-rows, its first nbytes / nsub / nhid elements (the lengths of the intensity, the subpixel and the hidden_points
    payloads; nhid cuts the 'hidden_points' column alike); 'nseq' and 'nnz' columns lie packed back to back, frame b at the sum of
    the counts before it.  nrow = max(seg) + 1 (tools/compress.py:102) = 1 + the index of the last non-zero count; 0 for a row of zeros,
    which no frame has (its counts sum to P)."""
    if torch.is_tensor(counts):
        xp, i64, ar = torch, (lambda v: v.to(torch.int64)), (lambda lo, hi: torch.arange(lo, hi, dtype=torch.int64, device=counts.device))
    else:
        xp, i64, ar = np, (lambda v: np.asarray(v, np.int64)), (lambda lo, hi: np.arange(lo, hi, dtype=np.int64))
    B, K = counts.shape
    n = {"nrow": xp.amax(i64(counts != 0) * ar(1, K + 1), 1), "nseq": i64(nseq), "nnz": i64(nnz), "nbytes": None if nbytes is None else i64(nbytes),
         "nsub": None if nsub is None else i64(nsub), "nhid": None if nhid is None else i64(nhid)}
    out = {}
    for c in cols:
        if c.cut in ("nseq", "nnz"):
            out[c.name] = (xp.cumsum(n[c.cut], 0) - n[c.cut], n[c.cut])
            continue
        shape = tuple(buffers[c.name].shape)
        row, sub = int(np.prod(shape[1:])), int(np.prod(shape[2:]))
        out[c.name] = (ar(0, B) * row, ar(0, B) * 0 + row if c.cut == "row" else n[c.cut] * sub)
    return out


class BatchPayload:
    """What the container of every frame of a batch is assembled from: views into the batch's host buffers -- a streaming slot's pinned
    ones or the arrays BatchCompressor.collect read back -- cut by frame_slices.  cols: columns(...); buffers, counts, nnz, nseq, nbytes, nsub, nhid:
    frame_slices' (numpy), the buffers read as the columns' dtypes; n: the frames that count (the first n; default all).
    frame(b) -> the dict compress_point_cloud builds (utils/compress_utils.py:138-179), before the entropy coder: views, no copies."""

    def __init__(self, cols, buffers, counts, nnz, nseq, nbytes=None, n=None, nsub=None, nhid=None):
        self.n = len(nnz) if n is None else n
        at = frame_slices(cols, buffers, counts, nnz, nseq, nbytes, nsub, nhid)
        # per column: the flattened buffer, the frames' first and last + 1 elements, the shape of a sub-row (the model's rows keep their [., 4])
        self.parts = [(c.name, buffers[c.name].reshape(-1).view(c.dtype), lo.tolist(), (lo + n_el).tolist(), (-1,) + tuple(buffers[c.name].shape[2:]))
                      for c in cols for lo, n_el in (at[c.name],)]

    def frame(self, b):
        return {name: flat[lo[b]: hi[b]].reshape(shape) for name, flat, lo, hi, shape in self.parts}

    def __len__(self):
        return self.n


def intensity_payload(q, scale):
    """The 'intensity' array of a frame: b"RPI1" | scale as little-endian float32 | q uint8 [n] of the non-empty pixels in raster order."""
    return np.frombuffer(INTENSITY_MAGIC + struct.pack("<f", scale) + np.ascontiguousarray(q, dtype=np.uint8).tobytes(), dtype=np.uint8)


def parse_intensity_payload(data, n):
    """-> (scale, q uint8 [n]) of a decoded 'intensity' array; ValueError unless it starts with the magic, carries a finite scale > 0 and
    holds exactly 8 + n bytes (n: the pixels whose label is not 1)."""
    data = bytes(data)
    if len(data) < 8 or data[:4] != INTENSITY_MAGIC:
        raise ValueError("intensity payload: no %r header (%d bytes)" % (INTENSITY_MAGIC, len(data)))
    scale = np.frombuffer(data, dtype="<f4", count=1, offset=4)[0]
    if not (np.isfinite(scale) and scale > 0):
        raise ValueError("intensity payload: scale %r is not finite and > 0" % float(scale))
    if len(data) != 8 + n:
        raise ValueError("intensity payload: %d bytes for %d non-empty pixels (8 + %d expected)" % (len(data), n, n))
    return np.float32(scale), np.frombuffer(data, dtype=np.uint8, offset=8)


def intensity_trailer_span(blob, uniform=True):
    """(start, end) of the coded 'intensity' bytes of a container, or None: what follows the known payloads must be exactly one
    [int32 length | bytes] that ends the blob."""
    spans = list(payload_spans(blob, len(columns(uniform, True))))
    if len(spans) < len(columns(uniform, True)) or sum(spans[-1]) != len(blob):
        return None
    return spans[-1][0], sum(spans[-1])


BEAM_TABLE_INTENSITY = ("intensity with a per-beam elevation table (channel_distribute_csv): that projection's rule is 'the last point wins', "
                        "another owner rule than the intensity kernels'; use a lidar configuration with evenly spaced beams")


def encode_intensity(transformer, rows, range_image, scale, want_image=False):
    """One frame's 'intensity' array on the per-frame path: rows [N,>=4] (host), range_image [H,W] the image of these rows (host array or
    device tensor) -> (uint8 [8 + n], the u8 [H,W] image of quantised values or None), by ops.intensity_encode."""
    if getattr(transformer, "even_dist", True) is False:
        raise NotImplementedError(BEAM_TABLE_INTENSITY)
    dev, H, W = transformer.device, transformer.H, transformer.W
    rows = np.asarray(rows)
    if rows.ndim != 2 or rows.shape[1] < 4:
        raise ValueError("intensity: the frame holds %s values per point, no intensity column" % (rows.shape[1] if rows.ndim == 2 else "?"))
    rows_d = torch.from_numpy(np.ascontiguousarray(rows[:, :4], dtype=np.float32)).to(dev)
    ri = range_image if torch.is_tensor(range_image) else torch.from_numpy(np.ascontiguousarray(range_image, dtype=np.float32)).to(dev)
    offs = torch.tensor([0, rows_d.shape[0]], dtype=torch.int64, device=dev)
    payload, nbytes, image, orphans = ops.intensity_encode(rows_d, offs, transformer.geom, ri.reshape(1, H, W).contiguous(), scale, want_image=want_image)
    if int(orphans[0]):
        raise RuntimeError("intensity: %d non-empty pixels have no owner -- the range image is not the image of these rows" % int(orphans[0]))
    return payload[0, : int(nbytes[0])].cpu().numpy(), (image[0].cpu().numpy() if want_image else None)


BEAM_TABLE_SUBPIXEL = ("subpixel with a per-beam elevation table (channel_distribute_csv): that projection's rule is 'the last point wins' and "
                       "its rows are a search over the table, another owner rule and another row offset than the subpixel kernels'; use a lidar "
                       "configuration with evenly spaced beams")


def subpixel_payload(az, el, bits):
    """The 'subpixel' array of a frame: b"RPS1" | bits | 0 0 0 | az codes uint8 [n] | el codes uint8 [n] of the non-empty pixels in raster order."""
    az, el = np.ascontiguousarray(az, dtype=np.uint8).reshape(-1), np.ascontiguousarray(el, dtype=np.uint8).reshape(-1)
    if az.shape != el.shape:
        raise ValueError("subpixel payload: %d az codes, %d el codes" % (az.shape[0], el.shape[0]))
    return np.frombuffer(SUBPIXEL_MAGIC + bytes([ops.check_subpixel_bits(bits), 0, 0, 0]) + az.tobytes() + el.tobytes(), dtype=np.uint8)


def parse_subpixel_payload(data, n):
    """-> (bits, az uint8 [n], el uint8 [n]) of a decoded 'subpixel' array; ValueError unless it starts with the magic, names 1 .. 4 bits,
    has three zero bytes behind them, holds exactly 8 + 2n bytes (n: the pixels whose label is not 1) and no code >= 1 << bits."""
    data = bytes(data)
    if len(data) < 8 or data[:4] != SUBPIXEL_MAGIC:
        raise ValueError("subpixel payload: no %r header (%d bytes)" % (SUBPIXEL_MAGIC, len(data)))
    bits = data[4]
    if not 1 <= bits <= 4:
        raise ValueError("subpixel payload: %d bits per axis (1 .. 4)" % bits)
    if data[5:8] != b"\0\0\0":
        raise ValueError("subpixel payload: reserved bytes %r are not 0" % data[5:8])
    if len(data) != 8 + 2 * n:
        raise ValueError("subpixel payload: %d bytes for %d non-empty pixels (8 + 2 * %d expected)" % (len(data), n, n))
    codes = np.frombuffer(data, dtype=np.uint8, offset=8)
    if codes.size and int(codes.max()) >= 1 << bits:
        raise ValueError("subpixel payload: code %d at %d bits" % (int(codes.max()), bits))
    return bits, codes[:n], codes[n:]


def encode_subpixel(transformer, rows, range_image, bits, want_codes=False):
    """One frame's 'subpixel' array on the per-frame path: rows [N,>=3] (host), range_image [H,W] the image of these rows (host array or
    device tensor) -> (uint8 [8 + 2n], the u8 [H,W,2] (az, el) codes or None), by ops.subpixel_encode."""
    if getattr(transformer, "even_dist", True) is False:
        raise NotImplementedError(BEAM_TABLE_SUBPIXEL)
    dev, H, W = transformer.device, transformer.H, transformer.W
    rows_d = torch.from_numpy(rows16(rows)).to(dev)
    ri = range_image if torch.is_tensor(range_image) else torch.from_numpy(np.ascontiguousarray(range_image, dtype=np.float32)).to(dev)
    offs = torch.tensor([0, rows_d.shape[0]], dtype=torch.int64, device=dev)
    payload, nbytes, codes, orphans = ops.subpixel_encode(rows_d, offs, transformer.geom, ri.reshape(1, H, W).contiguous(), bits, want_codes=want_codes)
    if int(orphans[0]):
        raise RuntimeError("subpixel: %d non-empty pixels have no owner -- the range image is not the image of these rows" % int(orphans[0]))
    return payload[0, : int(nbytes[0])].cpu().numpy(), (codes[0].cpu().numpy() if want_codes else None)


BEAM_TABLE_HIDDEN = ("hidden_points with a per-beam elevation table (channel_distribute_csv): that projection's rule is 'the last point wins' and "
                     "its rows are a search over the table, another owner rule and another row offset than the hidden_points kernels'; use a lidar "
                     "configuration with evenly spaced beams")


def hidden_payload(bits, step, counts, k, az=None, el=None):
    """The 'hidden_points' array of a frame: b"RPH1" | bits | 0 0 0 | step f32 | m u32 | counts uint8 [n] of the non-empty pixels in raster
    order | the range codes as little-endian uint16 [m] | for bits > 0 the az codes uint8 [m] and the el codes uint8 [m]."""
    bits = ops.check_hidden_bits(bits)
    counts, k = np.ascontiguousarray(counts, dtype=np.uint8).reshape(-1), np.ascontiguousarray(k, dtype="<u2").reshape(-1)
    if int(counts.sum(dtype=np.int64)) != k.shape[0]:
        raise ValueError("hidden_points payload: the counts sum to %d, %d range codes" % (int(counts.sum(dtype=np.int64)), k.shape[0]))
    body = counts.tobytes() + k.tobytes()
    if bits:
        az, el = np.ascontiguousarray(az, dtype=np.uint8).reshape(-1), np.ascontiguousarray(el, dtype=np.uint8).reshape(-1)
        if az.shape != k.shape or el.shape != k.shape:
            raise ValueError("hidden_points payload: %d range codes, %d az codes, %d el codes" % (k.shape[0], az.shape[0], el.shape[0]))
        body += az.tobytes() + el.tobytes()
    head = HIDDEN_MAGIC + bytes([bits, 0, 0, 0]) + struct.pack("<f", ops.check_hidden_step(step)) + struct.pack("<I", k.shape[0])
    return np.frombuffer(head + body, dtype=np.uint8)


def parse_hidden_payload(data, n):
    """-> (bits, step, counts uint8 [n], k uint16 [m], az uint8 [m], el uint8 [m]) of a decoded 'hidden_points' array; ValueError unless it
    holds a header, starts with the magic, names 0 .. 4 bits, has three zero bytes behind them, a finite step > 0, exactly 16 + n + 2m
    bytes (16 + n + 4m with lateral codes; n: the pixels whose label is not 1), counts that sum to m and no lateral code >= 1 << bits."""
    data = bytes(data)
    if len(data) < 16 or data[:4] != HIDDEN_MAGIC:
        raise ValueError("hidden_points payload: no %r header (%d bytes)" % (HIDDEN_MAGIC, len(data)))
    bits = data[4]
    if bits > 4:
        raise ValueError("hidden_points payload: %d bits per axis (0 .. 4)" % bits)
    if data[5:8] != b"\0\0\0":
        raise ValueError("hidden_points payload: reserved bytes %r are not 0" % data[5:8])
    step = np.frombuffer(data, dtype="<f4", count=1, offset=8)[0]
    if not (np.isfinite(step) and step > 0):
        raise ValueError("hidden_points payload: step %r is not finite and > 0" % float(step))
    (m,) = struct.unpack_from("<I", data, 12)
    w = 4 if bits else 2
    if len(data) != 16 + n + w * m:
        raise ValueError("hidden_points payload: %d bytes for %d non-empty pixels and %d points (16 + %d + %d * %d expected)" % (len(data), n, m, n, w, m))
    counts = np.frombuffer(data, dtype=np.uint8, count=n, offset=16)
    if int(counts.sum(dtype=np.int64)) != m:
        raise ValueError("hidden_points payload: the counts sum to %d, the header names %d points" % (int(counts.sum(dtype=np.int64)), m))
    k = np.frombuffer(data, dtype="<u2", count=m, offset=16 + n)
    lat = np.frombuffer(data, dtype=np.uint8, count=2 * m if bits else 0, offset=16 + n + 2 * m)
    if lat.size and int(lat.max()) >= 1 << bits:
        raise ValueError("hidden_points payload: code %d at %d bits" % (int(lat.max()), bits))
    return bits, np.float32(step), counts, k, (lat[:m] if bits else np.zeros(m, np.uint8)), (lat[m:] if bits else np.zeros(m, np.uint8))


def encode_hidden(transformer, rows, range_image, step, bits=0):
    """One frame's 'hidden_points' array on the per-frame path: rows [N,>=3] (host), range_image [H,W] the image of these rows (host array
    or device tensor), step the fp32 quantiser step, bits 0 .. 4 -> (uint8 [16 + n + 2m] or [16 + n + 4m], uncarried int), by ops.hidden_encode."""
    if getattr(transformer, "even_dist", True) is False:
        raise NotImplementedError(BEAM_TABLE_HIDDEN)
    dev, H, W = transformer.device, transformer.H, transformer.W
    rows_d = torch.from_numpy(rows16(rows)).to(dev)
    ri = range_image if torch.is_tensor(range_image) else torch.from_numpy(np.ascontiguousarray(range_image, dtype=np.float32)).to(dev)
    offs = torch.tensor([0, rows_d.shape[0]], dtype=torch.int64, device=dev)
    payload, nbytes, orphans, uncarried = ops.hidden_encode(rows_d, offs, transformer.geom, ri.reshape(1, H, W).contiguous(), step, bits,
                                                           max_rows=rows_d.shape[0])
    if int(orphans[0]):
        raise RuntimeError("hidden_points: %d non-empty pixels have no owner -- the range image is not the image of these rows" % int(orphans[0]))
    return payload[0, : int(nbytes[0])].cpu().numpy(), int(uncarried[0])


def rows16(points):
    """Host points [N,>=3] as the 16-byte rows f32 [N,4] the owner pass reads: the first four columns, or xyz and a zero fourth column."""
    points = np.asarray(points)
    if points.ndim != 2 or points.shape[1] < 3:
        raise ValueError("points [N,>=3] are needed, got %s" % (points.shape,))
    if points.shape[1] >= 4:
        return np.ascontiguousarray(points[:, :4], dtype=np.float32)
    out = np.zeros((points.shape[0], 4), np.float32)
    out[:, :3] = points
    return out


def pack_bitstream(compressed_data, uniform=True):
    """The .rpcc container (utils/compress_utils.py:167-179): [int32 length | bytes] per array; 'intensity', then 'subpixel', then
    'hidden_points', last where the dictionary holds them."""
    keys = _keys(uniform, compressed_data)
    return b"".join(struct.pack("i", len(compressed_data[k])) + bytes(compressed_data[k]) for k in keys)


def pack_frames(basic_compressor, frames, uniform=True):
    """The .rpcc byte strings of several frames: compress_dict + pack_bitstream per frame, with the bzip2 back-end done by
    ONE call into librpcc_host.so for the whole list (include/rpcc_host.h) -- a pool thread then enters the interpreter once
    per chunk of frames instead of once per array.  Same bytes as the per-frame path (tests/test_host_pack.py)."""
    from . import _lib
    host = None
    if basic_compressor.method_name == "bzip2" and frames:
        try:
            host = _lib.host_lib()     # not built / not loadable / stale: remembered by _lib, the Python path below gives the same bytes
        except _lib.RpccError:
            host = None
    if basic_compressor.batch_codec() and frames:   # every array of the chunk in one dumps_many / compress_many
        blobs = iter(basic_compressor.batch_codec()[1]([np.ascontiguousarray(od[k]) for od in frames for k in _keys(uniform, od)]))
        return [b"".join(struct.pack("i", len(b)) + b for b in (next(blobs) for _ in _keys(uniform, od))) for od in frames]
    if host is None or len({_keys(uniform, od) for od in frames}) > 1:   # (the host call takes one array count for the whole chunk)
        return [pack_bitstream(basic_compressor.compress_dict({k: od[k] for k in _keys(uniform, od)}), uniform=uniform) for od in frames]
    keys = _keys(uniform, frames[0])
    arrs = [np.ascontiguousarray(od[k]) for od in frames for k in keys]
    n, na = len(frames), len(keys)
    ptrs = np.fromiter((a.ctypes.data for a in arrs), dtype=np.uint64, count=n * na)
    lens = np.fromiter((a.nbytes for a in arrs), dtype=np.uint32, count=n * na)
    # bzip2 never expands by more than 1 % + 600 bytes; every frame gets the room its own arrays need
    room = (lens.reshape(n, na).astype(np.int64) * 101 // 100 + 604).sum(1)
    offs = np.zeros(n + 1, np.uint64)
    offs[1:] = np.cumsum(room)
    out = np.empty(int(offs[-1]), np.uint8)
    out_len = np.zeros(n, np.uint32)
    rc = host.rpcc_host_pack_bz2(n, na, ptrs.ctypes.data, lens.ctypes.data, out.ctypes.data, offs.ctypes.data, out_len.ctypes.data)
    if rc == -1:
        raise RuntimeError("rpcc_host_pack_bz2: bad argument")
    if rc != 0:
        raise RuntimeError("rpcc_host_pack_bz2 failed on frame %d of the chunk" % (-rc - 16))
    return [out[int(offs[i]): int(offs[i]) + int(out_len[i])].tobytes() for i in range(n)]


def unpack_bitstream(blob, uniform=True, intensity=False, subpixel=False, hidden_points=False):
    """intensity=True (a caller that asks for it): the dictionary also holds 'intensity', the coded trailer -- ValueError unless what
    follows the known payloads is exactly one length-prefixed payload that ends the blob.  Without it: trailing bytes are ignored, as ever.
    subpixel=True: 'subpixel' alike; hidden_points=True: 'hidden_points' alike.  The reader is told which trailers to expect: what follows the geometry must be exactly the trailers
    asked for, in file order, ending the blob -- ValueError naming the flag that does not fit otherwise."""
    keys = _keys(uniform)
    spans = list(payload_spans(blob, len(keys)))
    off = sum(spans[-1]) if spans else 0      # where the walk ended
    if len(spans) < len(keys):
        # (the reference reads whatever f.read(n) returns; a truncated or foreign file then fails somewhere inside the entropy decoder)
        k = keys[len(spans)]
        if off + 4 > len(blob):
            raise ValueError("bitstream ends before the length of '%s' (%d bytes; written with the %s framework?)"
                             % (k, len(blob), "non-uniform" if uniform else "uniform"))
        raise ValueError("bitstream: payload '%s' claims %d bytes, %d are left" % (k, struct.unpack_from("i", blob, off)[0], len(blob) - off - 4))
    out = {k: blob[s: s + n] for k, (s, n) in zip(keys, spans)}
    want = tuple(t for t, on in zip(TRAILERS, (intensity, subpixel, hidden_points)) if on)
    if not want:
        return out
    tail = list(payload_spans(blob, len(keys) + len(TRAILERS)))[len(keys):]      # the trailers the blob holds, three at most
    if len(tail) >= len(want) and sum(tail[len(want) - 1]) == len(blob):
        out.update({t: blob[s: s + n] for t, (s, n) in zip(want, tail)})
        return out
    if len(tail) > len(want) and sum(tail[-1]) == len(blob):                      # more trailers end the blob than were asked for
        if len(tail) == 2 and len(want) == 1 and want[0] in TRAILERS[:2]:         # one of the two older flags, two trailers: the text it always had,
            other = TRAILERS[1 - TRAILERS.index(want[0])]                         # and behind it the third flag, which explains such a blob as well
            raise ValueError("bitstream: two trailers follow its %d payloads and only %s was asked for (compressed with --%s too? the reader needs "
                             "%s=True then); or with --hidden_points: hidden_points=True" % (len(out), want[0], other, other))
        missing = [t for t in TRAILERS if t not in want]                          # every one of them, or one of them: the container names no payload
        glue =" and " if len(tail) - len(want) == len(missing) else " or "
        raise ValueError("bitstream: %s trailers follow its %d payloads and only %s asked for (compressed with --%s too? the reader needs "
                         "%s then)" % (("one", "two", "three")[len(tail) - 1], len(out), " and ".join(want) + (" was" if len(want) == 1 else " were"),
                                       (glue + "--").join(missing), glue.join(m + "=True" for m in missing)))
    if len(tail) >= len(want):
        raise ValueError("bitstream: %d bytes follow the %s trailer; the trailers asked for must end the container"
                         % (len(blob) - sum(tail[len(want) - 1]), want[-1]))
    flag = want[len(tail)]
    raise ValueError("bitstream: no %s trailer after its %d payloads (%d bytes follow them; compressed without --%s?)"
                     % (flag, len(out) + len(tail), len(blob) - (sum(tail[-1]) if tail else off), flag))


def save_compressed_bitstream(file, compressed_data, uniform=True):
    with open(file, "wb") as f:
        f.write(pack_bitstream(compressed_data, uniform))


def read_compressed_bitstream(file, uniform=True, intensity=False, subpixel=False, hidden_points=False):
    with open(file, "rb") as f:
        return unpack_bitstream(f.read(), uniform, intensity=intensity, subpixel=subpixel, hidden_points=hidden_points)


def decompress_point_cloud(compressed_data, basic_compressor, model_num, H, W):
    """utils/compress_utils.py:199-214 -> (residual_quantized int16, idx_map, salience_level, plane_param)."""
    d = basic_compressor.decompress_dict(compressed_data)
    plane_param = np.ndarray(shape=(model_num, 4), dtype=np.float32, buffer=d["plane_param"])
    contour_map = np.unpackbits(np.ndarray(shape=(-1,), dtype=np.uint8, buffer=d["contour_map"]))[: H * W].reshape(H, W)
    idx_sequence = np.ndarray(shape=(-1,), dtype=np.uint16, buffer=d["idx_sequence"])
    idx_map = ContourExtractor.recover_map(contour_map, idx_sequence)
    salience = np.ndarray(shape=(-1,), dtype=np.uint8, buffer=d["salience_level"]) if "salience_level" in d else None
    residual_quantized = np.ndarray(shape=(-1,), dtype=np.int16, buffer=d["residual_quantized"])
    return residual_quantized, idx_map, salience, plane_param


# One row per basic_compressor method: the host library's functions (None: there is none, the device modules are used whatever the flags
# say -- 'lz4' takes the lz4 package first where it is installed, see BasicCompressor._lz4), the device encoder --
# module of this package, its list encoder, the BasicCompressor flag that turns it on -- and the device decoder alike; work_slots: its
# decode_descriptors takes work slots; typed: its encode_descriptors takes each stream's element width (widths=) and filter (filters=).
# The modules are imported where a row is used, not here.
Backend = collections.namedtuple("Backend", "host_encode host_decode encoder encode_many encode_flag decoder decode_many decode_flag work_slots typed")
_GZIP = Backend(gzip.compress, gzip.decompress, "deflate_codec", "compress_many", "device_entropy", "inflate_codec", "decompress_many", "device_entropy", False, False)
BACKENDS = {
    "lz4": Backend(None, None, "lz4_codec", "dumps_many", None, "lz4_codec", "loads_many", None, False, False),
    "bzip2": Backend(bz2.compress, bz2.decompress, "bzip2_codec", "compress_many", "device_bzip2", "bunzip2_codec", "decompress_many", "device_bunzip2", True, False),
    "gzip": _GZIP,
    "deflate": _GZIP,
    "rans": Backend(None, None, "rans_codec", "compress_many", None, "rans_codec", "decompress_many", None, False, True),
}


def _module(name):
    return importlib.import_module("." + name, __package__)


def device_decoder(method_name):
    """What pipeline.BatchDecompressor asks of a method's device decoder: (work_bytes(a stream's first bytes, its cap) -> the bytes of its
    work slot, 0 where the decoder has none; decode_slots(descriptor rows [addr, lens, dst_off, dst_cap, work_off, work_cap], dst, work) ->
    (dst_len, status) GPU tensors, enqueued on the current stream)."""
    be = BACKENDS[method_name]
    codec = _module(be.decoder)
    if be.work_slots:
        return codec.stream_work_bytes, codec.decode_slots
    return (lambda head, cap: 0), (lambda d, dst, work: codec.decode_descriptors(d[0], d[1], dst, d[2], d[3]))


class BasicCompressor:
    """utils/compress_utils.py:232-310.  bzip2 / deflate are stdlib; lz4 is the lz4 package (lz4==0.7.0 API in the reference)
    where it is installed, else rpcc_amd.lz4_codec (the same dumps / loads forms, coded on the GPU).  device_entropy=True
    (opt-in) sends 'deflate' / 'gzip' through rpcc_amd.deflate_codec: gzip members coded on the GPU, other bytes than
    gzip.compress's, read by the same gzip.decompress -- and, under the same flag, by rpcc_amd.inflate_codec on the GPU.
    device_bunzip2=True (opt-in, a flag of its own) decodes 'bzip2' streams through rpcc_amd.bunzip2_codec on the GPU, with
    bz2.decompress's bytes.  device_bzip2=True (opt-in, a flag of its own) encodes 'bzip2' through rpcc_amd.bzip2_codec on the GPU:
    valid bzip2 streams of the build's own bytes, read by the same bz2.decompress.  Without that flag 'bzip2' is
    compressed by bz2.compress (or librpcc_host.so for a chunk of frames).  'rans' (the build's own format, not the reference's) is
    rpcc_amd.rans_codec on the GPU in both directions, whatever the flags say: it has no host coder.  rans_delta=True (opt-in, 'rans'
    only; nothing with any other method) codes the arrays rans_codec.delta_filter names -- the int16 residuals -- through the delta
    filter (format version 2); decoding takes no flag, both versions are read."""

    METHODS = ["lz4", "bzip2", "gzip", "deflate", "rans"]

    def __init__(self, compressor_yaml=None, method_name=None, device_entropy=False, device_bunzip2=False, device_bzip2=False, rans_delta=False):
        self.method_name = None
        self.device_entropy = bool(device_entropy)
        self.device_bunzip2 = bool(device_bunzip2)
        self.device_bzip2 = bool(device_bzip2)
        self.rans_delta = bool(rans_delta)
        if compressor_yaml is not None:
            self.method_name = load_yaml(compressor_yaml)["basic_compressor"]
        if method_name is not None:
            self.method_name = method_name
        if self.method_name is not None:
            assert self.method_name in self.METHODS, "Compression method is not existed. (lz4, bzip2, gzip, deflate, rans)"

    def set_method(self, method_name):
        assert method_name in self.METHODS, "Compression method is not existed. (lz4, bzip2, gzip, deflate, rans)"
        self.method_name = method_name

    def _resolved(self):
        """The one place that chooses the back-end, from BACKENDS: (method_name, flags) -> (compress one array, decompress one stream, (device
        encoder module, its list encoder) or None, the device decoder's list decoder or None).  No method set: four times None."""
        be = BACKENDS.get(self.method_name)
        if be is None:
            return None, None, None, None
        host, on = (be.host_encode, be.host_decode), lambda flag: getattr(self, flag)
        if be.host_encode is None:       # no host function in the row: its device modules, whatever the flags say ('rans', and 'lz4' ...
            pkg = self._lz4() if self.method_name == "lz4" else None      # ... unless the lz4 package is installed)
            if pkg is not None and pkg is not _module(be.encoder):
                host, on = (lambda a: pkg.dumps(a.tobytes()), pkg.loads), lambda flag: False
            else:
                on = lambda flag: True
        codec = (_module(be.encoder), getattr(_module(be.encoder), be.encode_many)) if on(be.encode_flag) else None
        if self.method_name == "rans" and self.rans_delta:    # the same module's list encoder with the delta filter where its rule gives one
            codec = (codec[0], codec[0].compress_many_delta)
        decoder = getattr(_module(be.decoder), be.decode_many) if on(be.decode_flag) else None
        return (lambda a: codec[1]([a])[0]) if codec else host[0], (lambda s: decoder([s])[0]) if decoder else host[1], codec, decoder

    def _batched(self, name):
        codec = self._resolved()[2]
        return codec is not None and codec[0].__name__.endswith("." + name)

    def lz4_batched(self):
        """True when 'lz4' runs through rpcc_amd.lz4_codec, which codes a list of arrays in one launch."""
        return self._batched("lz4_codec")

    def deflate_batched(self):
        """True when 'deflate' / 'gzip' runs through rpcc_amd.deflate_codec (device_entropy), which codes a list of arrays at once."""
        return self._batched("deflate_codec")

    def bzip2_batched(self):
        """True when 'bzip2' is encoded through rpcc_amd.bzip2_codec (device_bzip2), which codes a list of arrays at once."""
        return self._batched("bzip2_codec")

    def batch_codec(self):
        """(module, its list encoder) of the back-end that codes a list of arrays on the device at once, or None."""
        return self._resolved()[2]

    def compress_dict(self, data_dict):
        if self.batch_codec():
            return dict(zip(data_dict, self.batch_codec()[1]([np.ascontiguousarray(v) for v in data_dict.values()])))
        return {k: self.compress(v) for k, v in data_dict.items()}

    def batch_decoder(self):
        """The list decoder of the back-end that decodes a list of streams on the device at once, or None."""
        return self._resolved()[3]

    def decompress_dict(self, data_dict):
        if self.batch_decoder():
            return dict(zip(data_dict, self.batch_decoder()(list(data_dict.values()))))
        return {k: self.decompress(v) for k, v in data_dict.items()}

    def decompress_dicts(self, data_dicts):
        """decompress_dict over the frames of a chunk: every array of the chunk in one call where batch_decoder() exists."""
        data_dicts = list(data_dicts)
        if not self.batch_decoder() or not data_dicts:
            return [self.decompress_dict(d) for d in data_dicts]
        outs = iter(self.batch_decoder()([v for d in data_dicts for v in d.values()]))
        return [{k: next(outs) for k in d} for d in data_dicts]

    def compress(self, np_array):
        encode = self._resolved()[0]
        if encode is None:
            raise ValueError("no compression method set")
        return encode(np.ascontiguousarray(np_array))

    def decompress(self, bitstream):
        decode = self._resolved()[1]
        if decode is None:
            raise ValueError("no compression method set")
        return decode(bitstream)

    def calc_compressed_bytes(self, np_array):
        return len(self.compress(np_array))

    @staticmethod
    def _lz4():
        try:
            import lz4
            return lz4
        except ImportError:
            return _module("lz4_codec")
