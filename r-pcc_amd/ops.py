"""Stage-level Python wrappers of the C ABI (include/rpcc_hip.h): torch tensors in, torch tensors out.

PyTorch is only the device-memory container and the stream provider here; all compute is in
librpcc_hip.so.  Every function enqueues on torch's current HIP stream and does not synchronise.
"""
import ctypes as C
import functools
import math

import numpy as np
import torch

from . import _lib
from ._lib import Geom, BatchIO, check, ptr, stream

DEFAULT_CLUSTERS = 100


def make_geom(H, W, horizontal_FOV, vertical_max, vertical_min):
    """Geometry scalars as pybind11 hands them to the reference C++ (python doubles narrowed to float,
    cpp_modules.cpp:427-428)."""
    return Geom(int(H), int(W), float(horizontal_FOV), float(vertical_max), float(vertical_min))


def transform_map(H, W, horizontal_FOV, vertical_max, vertical_min, vertical_angle=None):
    """a1: PCTransformer.create_transform_map (dataset/transformer.py:41-54).  Frame-invariant host
    work (once per process): python-float cos/sin products rounded to fp32; the reference's H*W Python
    loop is evaluated as an outer product of the same fp64 factors.  vertical_angle (radians, one per row): the altitude
    of row h is vertical_angle[h] (the per-beam table, dataset/transformer.py:48) instead of the even spacing."""
    vfov = vertical_max - vertical_min
    if vertical_angle is not None:
        alt = [float(a) for a in beam_table(vertical_angle, H)]
    else:
        alt = [vfov * (h / (H - 1)) + vertical_min for h in range(H)]
    azi = [horizontal_FOV * (w / W) for w in range(W)]
    ca = np.array([math.cos(a) for a in alt]); sa = np.array([math.sin(a) for a in alt])
    cz = np.array([math.cos(a) for a in azi]); sz = np.array([math.sin(a) for a in azi])
    tm = np.zeros((H, W, 3))
    tm[..., 0] = ca[:, None] * cz[None, :]
    tm[..., 1] = ca[:, None] * sz[None, :]
    tm[..., 2] = sa[:, None]
    return tm.astype(np.float32)


def _dev(t):
    return t.device


def _point_stride(xyz):
    """Bytes per point of a point tensor: [N,3] packed xyz -> 12; [N,4] rows (x, y, z, intensity) as a KITTI .bin stores them
    (dataset/dataset.py:48-50) -> 16, read by the kernel as they are."""
    assert xyz.dim() == 2 and xyz.shape[1] in (3, 4) and xyz.dtype == torch.float32, "points: f32 [N,3] or [N,4]"
    return 4 * int(xyz.shape[1])


def beam_table(vertical_angle, H=None):
    """A per-beam elevation table as this build takes it: f64 [H] radians, row h of the image = entry h (any order, equal entries allowed).
    Refused by name, on the host: an entry that is NaN or +-inf, a length other than H (RANGE_IMAGE_HEIGHT), more than BEAM_MAX_H rows
    (the reference would raise IndexError or silently put points into wrong rows)."""
    va = np.ascontiguousarray(np.asarray(vertical_angle, dtype=np.float64).reshape(-1))
    if H is not None and va.shape[0] != int(H):
        raise ValueError("per-beam table: %d vertical angles for RANGE_IMAGE_HEIGHT = %d (one per row is needed)" % (va.shape[0], int(H)))
    if not 1 <= va.shape[0] <= _lib.BEAM_MAX_H:
        raise ValueError("per-beam table: %d rows; this build takes 1 .. %d (RPCC_BEAM_MAX_H)" % (va.shape[0], _lib.BEAM_MAX_H))
    if not np.isfinite(va).all():
        raise ValueError("per-beam table: entry %d is not finite" % int(np.flatnonzero(~np.isfinite(va))[0]))
    return va


def beam_index_host(vertical_angle):
    """The index of rpcc_project_beams for a table (rpcc_beam_index_build; layout: csrc/beam_index.h) as a uint8 array; built on the host,
    no device is touched."""
    va = beam_table(vertical_angle)
    H = va.shape[0]
    out = np.zeros(_lib.lib().rpcc_beam_index_bytes(H) // 8, dtype=np.float64)     # (8-byte aligned)
    check(_lib.lib().rpcc_beam_index_build(va.ctypes.data_as(C.c_void_p), H, out.ctypes.data_as(C.c_void_p)))
    return out.view(np.uint8)


def beam_index(vertical_angle, device):
    """beam_index_host() uploaded: what project(..., beams=) and compress_batch(..., beams=) take.  Once per transformer."""
    return torch.from_numpy(beam_index_host(vertical_angle).copy()).to(device)


def _check_beams(beams, geom):
    assert beams.dtype == torch.uint8 and beams.numel() == 24 * geom.H, "beams: the index built for this geometry's H (ops.beam_index)"


def project(xyz, offsets, geom, ri=None, scratch=None, atomic_path=False, beams=None):
    """a2 batched.  xyz f32 [total,3] -- or the stored rows f32 [total,4] (x, y, z, intensity), read with a 16-byte stride --,
    offsets i64 [B+1] (device) -> ri f32 [B,H,W].
    atomic_path=True gives the library only the small scratch, which selects the device-atomic kernels
    (same result as the default LDS-band kernels).
    beams (ops.beam_index): the projection through that per-beam elevation table instead (rpcc_project_beams: nearest table entry, the last point
    in input order wins its pixel; geom's two vertical angles are ignored and atomic_path has no meaning)."""
    B = offsets.numel() - 1
    P = geom.H * geom.W
    xyz = xyz.contiguous()
    if ri is None:
        ri = torch.empty((B, geom.H, geom.W), dtype=torch.float32, device=_dev(offsets))
    if beams is not None:
        _check_beams(beams, geom)
        if scratch is None:
            scratch = torch.empty(max(_lib.lib().rpcc_project_beams_scratch_bytes(xyz.shape[0], B, P), 1), dtype=torch.uint8, device=_dev(offsets))
        check(_lib.lib().rpcc_project_beams(ptr(xyz) if xyz.numel() else None, _point_stride(xyz), ptr(offsets), xyz.shape[0], B, geom,
                                            ptr(beams), ptr(ri), ptr(scratch), scratch.numel() * scratch.element_size(), stream()))
        return ri
    if scratch is None:
        n = B * (P + 8) * 4 if atomic_path else _lib.lib().rpcc_project_scratch_bytes(xyz.shape[0], B, P)
        scratch = torch.empty(n, dtype=torch.uint8, device=_dev(offsets))
    check(_lib.lib().rpcc_project_strided(ptr(xyz) if xyz.numel() else None, _point_stride(xyz), ptr(offsets), xyz.shape[0], B, geom,
                                          ptr(ri), ptr(scratch), scratch.numel() * scratch.element_size(), stream()))
    return ri


def project_fastpath_check(xyz, geom):
    """Test hook of a2: (points the screened fast path is certain about, of those the ones whose pixel differs
    from the exact sequence -- must be 0 --, points sent to the exact sequence, max column discrepancy, max row
    discrepancy of the pre-rounding coordinates [pixels])."""
    counts = torch.zeros((5,), dtype=torch.int64, device=_dev(xyz))
    check(_lib.lib().rpcc_project_fastpath_check(ptr(xyz), int(xyz.shape[0]), geom, ptr(counts), stream()))
    c = [int(v) for v in counts.cpu()]
    return c[0], c[1], c[2], c[3] * 1e-9, c[4] * 1e-9


def project_beams_check(xyz, geom, beams):
    """Test hook of the table projection: (points the screened fast path is certain about, of those the ones the exact sequence skips or puts
    into another pixel -- must be 0 --, points sent to the exact sequence).  xyz: packed f32 [N,3]."""
    _check_beams(beams, geom)
    assert xyz.dim() == 2 and xyz.shape[1] == 3 and xyz.dtype == torch.float32 and xyz.is_contiguous()
    counts = torch.zeros((3,), dtype=torch.int64, device=_dev(xyz))
    check(_lib.lib().rpcc_project_beams_check(ptr(xyz), int(xyz.shape[0]), geom, ptr(beams), ptr(counts), stream()))
    return tuple(int(v) for v in counts.cpu())


def check_intensity_scale(scale):
    """An intensity scale as the kernels take it: an fp32 value, finite and > 0."""
    with np.errstate(over="ignore"):
        s = float(np.float32(scale))
    if not (math.isfinite(s) and s > 0):
        raise ValueError("intensity scale %r: a finite float32 value > 0 is needed" % (scale,))
    return s


def intensity_encode(rows, offsets, geom, ri, scale, want_image=False, payload=None, nbytes=None, image=None, orphans=None, scratch=None,
                     owner_intensity=None):
    """The intensity payloads of a batch (rpcc_intensity_encode; specification: tests/intensity_ref.py).  rows f32 [total,4] (x, y, z,
    intensity), offsets i64 [B+1], ri f32 [B,H,W] the range image ops.project / the batch call made of THESE rows, scale finite > 0
    -> (payload u8 [B, 8+P]: b"RPI1" | scale f32 | one byte per non-empty pixel in raster order, nbytes i32 [B] = 8 + n,
    image u8 [B,H,W] or None, orphans i32 [B]: non-empty pixels no row owns -- 0 whenever ri is the image of these rows).
    The bytes of a payload row past nbytes are left as they were.  payload .. scratch: the caller's buffers.  owner_intensity: a caller's
    f32 [B,H,W] tensor that receives every pixel's owner's intensity as stored (0 where empty)."""
    if rows.dim() != 2 or rows.shape[1] != 4:
        raise ValueError("intensity_encode: rows [total,%s] hold no intensity column; the stored (x, y, z, intensity) rows [total,4] are needed"
                         % (rows.shape[1] if rows.dim() == 2 else "?"))
    assert rows.dtype == torch.float32 and ri.dtype == torch.float32
    scale = check_intensity_scale(scale)
    B, P, dev = offsets.numel() - 1, geom.H * geom.W, _dev(offsets)
    rows = rows.contiguous()
    if payload is None:
        payload = torch.empty((B, 8 + P), dtype=torch.uint8, device=dev)
    if nbytes is None:
        nbytes = torch.empty((B,), dtype=torch.int32, device=dev)
    if orphans is None:
        orphans = torch.empty((B,), dtype=torch.int32, device=dev)
    if want_image and image is None:
        image = torch.empty((B, geom.H, geom.W), dtype=torch.uint8, device=dev)
    if scratch is None:
        scratch = torch.empty(_lib.lib().rpcc_intensity_scratch_bytes(B, P), dtype=torch.uint8, device=dev)
    check(_lib.lib().rpcc_intensity_encode(ptr(rows) if rows.numel() else None, ptr(offsets), rows.shape[0], B, geom, ptr(ri), scale, ptr(payload),
                                           payload.stride(0), ptr(nbytes), ptr(image) if want_image else None, ptr(owner_intensity), ptr(orphans), ptr(scratch),
                                           scratch.numel(), stream()))
    return payload, nbytes, (image if want_image else None), orphans


def intensity_decode(payload, nbytes, seg, out=None, status=None):
    """The way back (rpcc_intensity_decode): payload u8 [B, >= 8+P] rows, nbytes i32 [B], seg [B,H,W] uint8 or uint16 label maps (label 1:
    an empty pixel) -> (intensity f32 [B,H,W], 0 where the label is 1; status i32 [B]: _lib.STREAM_OK, or _lib.STREAM_E_INTENSITY for a
    row without the magic, with a scale that is not finite and > 0 or with another byte count than 8 + (labels != 1): zeros)."""
    B, H, W = seg.shape
    assert payload.dtype == torch.uint8 and payload.dim() == 2 and payload.shape[0] == B and payload.stride(1) == 1
    assert seg.dtype in (torch.uint8, torch.uint16) and nbytes.dtype == torch.int32 and nbytes.numel() == B
    if out is None:
        out = torch.empty((B, H, W), dtype=torch.float32, device=_dev(seg))
    if status is None:
        status = torch.empty((B,), dtype=torch.int32, device=_dev(seg))
    check(_lib.lib().rpcc_intensity_decode(C.c_void_p(payload.data_ptr()), payload.stride(0), ptr(nbytes), ptr(seg), seg.element_size(), B, H * W,
                                           ptr(out), ptr(status), stream()))
    return out, status


SUBPIXEL_TABLE_CODES = 16     # SUB_TABLE_CODES (csrc/subpixel_kernels.h): codes per bits row of the decoder's table


def check_subpixel_bits(bits):
    """The code width of the subpixel channel as the kernels take it: an integer 1 .. 4 (bits per axis)."""
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 1 <= int(bits) <= 4:
        raise ValueError("subpixel bits %r: an integer 1 .. 4 is needed" % (bits,))
    return int(bits)


def subpixel_tables(H, W, horizontal_FOV, vertical_max, vertical_min):
    """The decoder's table of rpcc_subpixel_decode (include/rpcc_hip.h), f64 [2H + 2W + 256], built from python floats as transform_map
    builds its factors: cos / sin of every row's altitude and every column's azimuth, then for bits 1 .. 4 and every code the cos / sin of
    the elevation step and of the azimuth step the code stands for."""
    vfov = vertical_max - vertical_min
    alt = [vfov * (h / (H - 1)) + vertical_min for h in range(H)]
    azi = [horizontal_FOV * (w / W) for w in range(W)]
    out = [math.cos(a) for a in alt] + [math.sin(a) for a in alt] + [math.cos(a) for a in azi] + [math.sin(a) for a in azi]
    for bits in (1, 2, 3, 4):
        L = 1 << bits
        for c in range(SUBPIXEL_TABLE_CODES):
            de = ((c + 0.5) / L - 0.5) * (vfov / (H - 1))
            da = ((c + 0.5) / L - 0.5) * (horizontal_FOV / W)
            out += [math.cos(de), math.sin(de), math.cos(da), math.sin(da)] if c < L else [0.0] * 4
    return np.array(out, dtype=np.float64)


def subpixel_encode(rows, offsets, geom, ri, bits, want_codes=False, payload=None, nbytes=None, codes=None, orphans=None, scratch=None):
    """The subpixel payloads of a batch (rpcc_subpixel_encode; specification: tests/subpixel_ref.py).  rows f32 [total,4] (x, y, z and a
    fourth column that is not read), offsets i64 [B+1], ri f32 [B,H,W] the range image ops.project / the batch call made of THESE rows,
    bits 1 .. 4 -> (payload u8 [B, 8+2P]: b"RPS1" | bits | 0 0 0 | the az codes of the non-empty pixels in raster order | their el codes,
    nbytes i32 [B] = 8 + 2n, codes u8 [B,H,W,2] or None, orphans i32 [B]: non-empty pixels no row owns -- 0 whenever ri is the image of
    these rows).  The bytes of a payload row past nbytes are left as they were.  payload .. scratch: the caller's buffers."""
    if rows.dim() != 2 or rows.shape[1] != 4:
        raise ValueError("subpixel_encode: rows [total,%s]; the stored 16-byte rows [total,4] are needed (packed xyz: add a zero column)"
                         % (rows.shape[1] if rows.dim() == 2 else "?"))
    assert rows.dtype == torch.float32 and ri.dtype == torch.float32
    bits = check_subpixel_bits(bits)
    B, P, dev = offsets.numel() - 1, geom.H * geom.W, _dev(offsets)
    rows = rows.contiguous()
    if payload is None:
        payload = torch.empty((B, 8 + 2 * P), dtype=torch.uint8, device=dev)
    if nbytes is None:
        nbytes = torch.empty((B,), dtype=torch.int32, device=dev)
    if orphans is None:
        orphans = torch.empty((B,), dtype=torch.int32, device=dev)
    if want_codes and codes is None:
        codes = torch.empty((B, geom.H, geom.W, 2), dtype=torch.uint8, device=dev)
    if scratch is None:
        scratch = torch.empty(_lib.lib().rpcc_subpixel_scratch_bytes(B, P), dtype=torch.uint8, device=dev)
    check(_lib.lib().rpcc_subpixel_encode(ptr(rows) if rows.numel() else None, ptr(offsets), rows.shape[0], B, geom, ptr(ri), bits, ptr(payload),
                                          payload.stride(0), ptr(nbytes), ptr(codes) if want_codes else None, ptr(orphans), ptr(scratch),
                                          scratch.numel(), stream()))
    return payload, nbytes, (codes if want_codes else None), orphans


def subpixel_decode(payload, nbytes, seg, ri_rec, tables, out=None, status=None):
    """The way back (rpcc_subpixel_decode): payload u8 [B, >= 8+2P] rows, nbytes i32 [B], seg [B,H,W] uint8 or uint16 label maps (label 1:
    an empty pixel), ri_rec f32 [B,H,W] the reconstructed ranges, tables f64 the device copy of subpixel_tables (PCTransformer.subpixel_tables)
    -> (points f32 [B,H,W,3], +0.0 where the label is 1; status i32 [B]: _lib.STREAM_OK, or _lib.STREAM_E_SUBPIXEL for a refused row: zeros)."""
    B, H, W = seg.shape
    assert payload.dtype == torch.uint8 and payload.dim() == 2 and payload.shape[0] == B and payload.stride(1) == 1
    assert seg.dtype in (torch.uint8, torch.uint16) and nbytes.dtype == torch.int32 and nbytes.numel() == B
    assert ri_rec.dtype == torch.float32 and ri_rec.numel() == B * H * W
    assert tables.dtype == torch.float64 and tables.numel() == 2 * H + 2 * W + 4 * SUBPIXEL_TABLE_CODES * 4, "tables: PCTransformer.subpixel_tables() of this geometry"
    if out is None:
        out = torch.empty((B, H, W, 3), dtype=torch.float32, device=_dev(seg))
    if status is None:
        status = torch.empty((B,), dtype=torch.int32, device=_dev(seg))
    check(_lib.lib().rpcc_subpixel_decode(C.c_void_p(payload.data_ptr()), payload.stride(0), ptr(nbytes), ptr(seg), seg.element_size(), ptr(ri_rec),
                                          ptr(tables), H, W, B, ptr(out), ptr(status), stream()))
    return out, status


HIDDEN_HEADER = 16            # HID_HEADER (csrc/hidden_kernels.h): magic, bits, reserved, step, m


def check_hidden_bits(bits):
    """The lateral code width of the hidden_points channel: an integer 0 .. 4 (0: range codes only)."""
    if isinstance(bits, bool) or not isinstance(bits, (int, np.integer)) or not 0 <= int(bits) <= 4:
        raise ValueError("hidden_points bits %r: an integer 0 .. 4 is needed" % (bits,))
    return int(bits)


def check_hidden_step(step):
    """The quantiser step of the hidden_points channel as the kernels take it: an fp32 value, finite and > 0."""
    with np.errstate(over="ignore"):
        s = float(np.float32(step))
    if not (math.isfinite(s) and s > 0):
        raise ValueError("hidden_points step %r: a finite float32 value > 0 is needed" % (step,))
    return s


def hidden_row_bytes(P, rows):
    """The longest hidden_points payload of a frame of `rows` input rows: 16 + P + 4 rows."""
    return HIDDEN_HEADER + int(P) + 4 * int(rows)


def hidden_encode(rows, offsets, geom, ri, step, bits=0, max_rows=None, payload=None, nbytes=None, orphans=None, uncarried=None, scratch=None):
    """The hidden_points payloads of a batch (rpcc_hidden_encode; specification: tests/hidden_ref.py).  rows f32 [total,4] (x, y, z and a
    fourth column that is not read), offsets i64 [B+1], ri f32 [B,H,W] the range image ops.project / the batch call made of THESE rows,
    step the fp32 quantiser step, bits 0 .. 4 the lateral code width -> (payload u8 [B, 16 + P + 4 max_rows]: b"RPH1" | bits | 0 0 0 |
    step f32 | m u32 | a count byte per non-empty pixel in raster order | the range codes u16 [m] | for bits > 0 the az codes [m] and the
    el codes [m]; nbytes i32 [B] = 16 + n + 2m or 16 + n + 4m; orphans i32 [B]; uncarried i32 [B]: hidden points in an empty pixel, past
    range code 65535 or past the 255 of their pixel).  max_rows: the rows of the batch's largest frame (None: read from offsets, one
    synchronisation).  The bytes of a payload row past nbytes are left as they were.  payload .. scratch: the caller's buffers."""
    if rows.dim() != 2 or rows.shape[1] != 4:
        raise ValueError("hidden_encode: rows [total,%s]; the stored 16-byte rows [total,4] are needed (packed xyz: add a zero column)"
                         % (rows.shape[1] if rows.dim() == 2 else "?"))
    assert rows.dtype == torch.float32 and ri.dtype == torch.float32
    step, bits = check_hidden_step(step), check_hidden_bits(bits)
    B, P, dev = offsets.numel() - 1, geom.H * geom.W, _dev(offsets)
    rows = rows.contiguous()
    if payload is None:
        if max_rows is None:
            max_rows = int((offsets[1:] - offsets[:-1]).max()) if B > 0 else 0
        payload = torch.empty((B, hidden_row_bytes(P, max(int(max_rows), 0))), dtype=torch.uint8, device=dev)
    if nbytes is None:
        nbytes = torch.empty((B,), dtype=torch.int32, device=dev)
    if orphans is None:
        orphans = torch.empty((B,), dtype=torch.int32, device=dev)
    if uncarried is None:
        uncarried = torch.empty((B,), dtype=torch.int32, device=dev)
    if scratch is None:
        scratch = torch.empty(_lib.lib().rpcc_hidden_scratch_bytes(B, P, rows.shape[0]), dtype=torch.uint8, device=dev)
    check(_lib.lib().rpcc_hidden_encode(ptr(rows) if rows.numel() else None, ptr(offsets), rows.shape[0], B, geom, ptr(ri), step, bits, ptr(payload),
                                        payload.stride(0), ptr(nbytes), ptr(orphans), ptr(uncarried), ptr(scratch), scratch.numel(), stream()))
    return payload, nbytes, orphans, uncarried


def hidden_decode(payload, nbytes, seg, tm, tables=None, capacity=None, out=None, count=None, status=None):
    """The way back (rpcc_hidden_decode): payload u8 [B, .] rows, nbytes i32 [B], seg [B,H,W] uint8 or uint16 label maps (label 1: an empty
    pixel), tm f32 [H,W,3] the transform map (PCTransformer.tm_dev), tables f64 the device copy of subpixel_tables or None (a frame with
    lateral codes is then refused) -> (points f32 [B, capacity, 3]: frame b's count[b] points in payload order, the rest left as it is;
    count i32 [B]; status i32 [B]: _lib.STREAM_OK, or _lib.STREAM_E_HIDDEN for a refused row: count 0, nothing written).  capacity: the
    most points a frame may hold (None: what the longest row could, (row bytes - 16) / 2)."""
    B, H, W = seg.shape
    assert payload.dtype == torch.uint8 and payload.dim() == 2 and payload.shape[0] == B and payload.stride(1) == 1
    assert seg.dtype in (torch.uint8, torch.uint16) and nbytes.dtype == torch.int32 and nbytes.numel() == B
    assert tm.dtype == torch.float32 and tm.numel() == H * W * 3 and tm.is_contiguous()
    if tables is not None:
        assert tables.dtype == torch.float64 and tables.numel() == 2 * H + 2 * W + 4 * SUBPIXEL_TABLE_CODES * 4, "tables: PCTransformer.subpixel_tables() of this geometry"
    if out is not None:
        capacity = out.shape[1]
    elif capacity is None:
        capacity = max((payload.shape[1] - HIDDEN_HEADER) // 2, 0)
    if out is None:
        out = torch.empty((B, capacity, 3), dtype=torch.float32, device=_dev(seg))
    assert out.dtype == torch.float32 and out.shape == (B, capacity, 3) and out.is_contiguous()
    if count is None:
        count = torch.empty((B,), dtype=torch.int32, device=_dev(seg))
    if status is None:
        status = torch.empty((B,), dtype=torch.int32, device=_dev(seg))
    row = payload.stride(0) if B > 1 else payload.shape[1]     # (the stride of a dimension of one frame says nothing)
    check(_lib.lib().rpcc_hidden_decode(C.c_void_p(payload.data_ptr()), row, ptr(nbytes), ptr(seg), seg.element_size(), ptr(tm),
                                        ptr(tables), H, W, B, ptr(out) if capacity else None, capacity, ptr(count), ptr(status), stream()))
    return out, count, status


def _frame_ids(frame_ids, B, device):
    """Stable per-frame identities (datalist indices) as a device i64 [B] tensor, or None."""
    if frame_ids is None:
        return None
    if not torch.is_tensor(frame_ids):
        frame_ids = torch.as_tensor(np.asarray(frame_ids, dtype=np.int64))
    frame_ids = frame_ids.to(device=device, dtype=torch.int64).contiguous()
    assert frame_ids.numel() == B, "one identity per frame"
    return frame_ids


def ground_ransac(ri, tm, seed=0, frame_ids=None):
    """a4: seeded ground-plane RANSAC -> (ground f64 [B,4], inlier counts i32 [B]).  Frame b draws with
    seed + frame_ids[b] (its datalist index; default: its position b in the batch)."""
    B = ri.shape[0]
    P = ri[0].numel()
    ground = torch.empty((B, 4), dtype=torch.float64, device=_dev(ri))
    inl = torch.empty((B,), dtype=torch.int32, device=_dev(ri))
    fid = _frame_ids(frame_ids, B, _dev(ri))
    check(_lib.lib().rpcc_ground_ransac(ptr(ri), ptr(tm), B, P, int(seed) & 0xFFFFFFFF, ptr(fid), ptr(ground), ptr(inl),
                                        stream()))
    return ground, inl


def ground_mask(ri, tm, ground, threshold, fps_table=False, table=None):
    """a3+a5.  -> (temp f32 [B,P], info i32 [B,8] = n_left, first candidate pixel, nnz, table flag, first empty
    candidate pixel, 3 spare).
    fps_table=True: the kernel also runs the first FPS pass and returns the tile table as third value
    (hand it to fps_range); results are identical either way.  table: the caller's buffer of rpcc_fps_table_bytes(B, H, W) bytes for it."""
    B, H, W = ri.shape
    P = H * W
    temp = torch.empty((B, P), dtype=torch.float32, device=_dev(ri))
    info = torch.empty((B, _lib.INFO_INTS), dtype=torch.int32, device=_dev(ri))
    tab = None
    if fps_table:
        tab = torch.empty(_lib.lib().rpcc_fps_table_bytes(B, H, W) // 4, dtype=torch.float32, device=_dev(ri)) if table is None else table
    check(_lib.lib().rpcc_ground_mask(ptr(ri), ptr(tm), ptr(ground), float(threshold), B, H, W, ptr(temp), ptr(info),
                                      ptr(tab), stream()))
    return (temp, info, tab) if fps_table else (temp, info)


def fps_xyz(points, npoint, temp=None, bruteforce=False, fma=0, cuda_tie=False):
    """a6 on an explicit point list: furthest_point_sampling_wrapper(b,n,m,points,temp,idx)
    (ops/fps/src/sampling.cpp:24-37).  points f32 [B,N,3] -> idx i32 [B,npoint].  bruteforce=True: the
    one-pass-per-centre kernel (test reference of the tile-pruned one; identical results).  fma / cuda_tie: the CUDA
    binary's contraction of sampling_gpu.cu:64 and its reduction tree's tie rule (_lib.fps_mode_flags; None = environment)."""
    B, N, _ = points.shape
    if temp is None:
        temp = torch.full((B, N), 1e10, dtype=torch.float32, device=_dev(points))
    idx = torch.empty((B, npoint), dtype=torch.int32, device=_dev(points))
    mode = _lib.fps_mode_flags(fma, cuda_tie)
    if mode:
        check(_lib.lib().rpcc_fps_xyz_mode(B, N, npoint, ptr(points), ptr(temp), ptr(idx), mode, stream()))
        return idx
    fn = _lib.lib().rpcc_fps_xyz_bruteforce if bruteforce else _lib.lib().rpcc_fps_xyz
    check(fn(B, N, npoint, ptr(points), ptr(temp), ptr(idx), stream()))
    return idx


def fps_xyz_probe(points):
    """Which kernel fps_xyz gives each list of points f32 [B,N,3]: i32 [B], -1 = one pass per centre (no locality in the point order),
    0 = tile-pruned (consecutive points are neighbours).  Test hook; the indices are the same either way."""
    B, N, _ = points.shape
    marks = torch.empty((B,), dtype=torch.int32, device=_dev(points))
    check(_lib.lib().rpcc_fps_xyz_probe(B, N, ptr(points), ptr(marks), stream()))
    return marks


def fps_range(ri, tm, temp, info, M, fps_table=None, cen_pix=None, centers=None, bruteforce=False, fma=0, cuda_tie=False):
    """a6 on the range image.  fma / cuda_tie: the CUDA-binary modes (_lib.fps_mode_flags); they need temp / info from
    ground_mask(..., fps_table=False)."""
    B, H, W = ri.shape
    cen_pix = torch.empty((B, M), dtype=torch.int32, device=_dev(ri)) if cen_pix is None else cen_pix
    centers = torch.empty((B, M, 3), dtype=torch.float32, device=_dev(ri)) if centers is None else centers
    flags = (_lib.FPS_BRUTEFORCE if bruteforce else 0) | _lib.fps_mode_flags(fma, cuda_tie)
    check(_lib.lib().rpcc_fps_range(ptr(ri), ptr(tm), ptr(temp), ptr(info), B, H, W, M, ptr(cen_pix), ptr(centers),
                                    flags, ptr(fps_table), stream()))
    return cen_pix, centers


def _stage_entry(name, M, seg=None):
    """The stage entry `name` for cluster count M: the byte-label one up to 254, its uint16 form (`name`_wide) up to 1022 -- and the label tensor's dtype
    must be the one the entry reads."""
    wide = is_wide(M)
    if wide and M > _lib.MAX_CLUSTERS_MID:
        check_cluster_num(M, stage="mid")
    if seg is not None:
        assert seg.dtype == (torch.uint16 if wide else torch.uint8), "labels of cluster_num = %d are %s on the device" % (M, "uint16" if wide else "uint8")
    return getattr(_lib.lib(), name + "_wide" if wide else name)


def label_dtype(M):
    return torch.uint16 if is_wide(M) else torch.uint8


def assign(ri, tm, ground, centers, out=None):
    """a7 -> labels u8 [B,H,W] (uint16 for 255 .. 1022 centres: rpcc_assign_wide)."""
    B, H, W = ri.shape
    M = centers.shape[1]
    seg = torch.empty((B, H, W), dtype=label_dtype(M), device=_dev(ri)) if out is None else out
    check(_stage_entry("rpcc_assign", M, seg)(ptr(ri), ptr(tm), ptr(ground), ptr(centers), B, H, W, M, ptr(seg), stream()))
    return seg


def workspace(B, P, M, device, total_points=0, general=False):
    """Work buffer of the fused entry; general=True: large enough for the plane model / the non-uniform framework too."""
    fn = _lib.lib().rpcc_wide_workspace_bytes if is_wide(M) else _lib.lib().rpcc_workspace_bytes_general if general else _lib.lib().rpcc_workspace_bytes
    n = fn(B, P, M, int(total_points))
    return torch.empty((n + 255) // 256 * 256, dtype=torch.uint8, device=device)


def point_model(ri, seg, ground, M, ws=None):
    B = ri.shape[0]
    P = ri[0].numel()
    K = M + 2
    ws = workspace(B, P, M, _dev(ri)) if ws is None else ws
    model = torch.empty((B, K, 4), dtype=torch.float32, device=_dev(ri))
    counts = torch.empty((B, K), dtype=torch.int32, device=_dev(ri))
    check(_stage_entry("rpcc_point_model", M, seg)(ptr(ri), ptr(seg), ptr(ground), B, P, M, ptr(model), ptr(counts), ptr(ws), stream()))
    return model, counts


def predict_quantize(ri, tm, seg, model, acc, M, want_pred=False, int16=False, ws=None, label_acc=None,
                     residual=None, q_out=None, nnz_out=None):
    """a10+a11(+a13).  label_acc f32 [B,K]: per-label steps (non-uniform); residual f32 [B,P]: use this
    residual instead of ri - pred.  -> (q [B,P] label-ordered, nnz [B], pred or None).  q_out / nnz_out: write into
    these buffers (entries of q past nnz are left as they are) instead of fresh ones.  The fresh q is zero-filled
    for the caller's sake only (a defined tail behind nnz): the library neither reads q nor needs it cleared
    (include/rpcc_hip.h "Caller's buffers")."""
    B = ri.shape[0]
    P = ri[0].numel()
    ws = workspace(B, P, M, _dev(ri)) if ws is None else ws
    if q_out is not None:
        assert q_out.dtype == (torch.int16 if int16 else torch.int32) and q_out.numel() == B * P
    q = torch.zeros((B, P), dtype=torch.int16 if int16 else torch.int32, device=_dev(ri)) if q_out is None else q_out
    nnz = torch.empty((B,), dtype=torch.int32, device=_dev(ri)) if nnz_out is None else nnz_out
    pred = torch.empty((B, P), dtype=torch.float32, device=_dev(ri)) if want_pred else None
    check(_stage_entry("rpcc_predict_quantize", M, seg)(ptr(ri), ptr(tm), ptr(seg), ptr(model), ptr(label_acc), ptr(residual),
                                                        float(acc), B, P, M, ptr(q) if int16 else None,
                                                        None if int16 else ptr(q), ptr(nnz), ptr(pred), ptr(ws), stream()))
    return q, nnz, pred


def intra_predict(seg, model, tm):
    """a10 alone -> pred f32 [B,H,W]."""
    B = seg.shape[0]
    P = seg[0].numel()
    pred = torch.empty(tuple(seg.shape), dtype=torch.float32, device=_dev(seg))
    fn = _lib.lib().rpcc_intra_predict_wide if seg.dtype == torch.uint16 else _lib.lib().rpcc_intra_predict    # (any label count: a row lookup per pixel)
    check(fn(ptr(seg), ptr(model), ptr(tm), B, P, model.shape[1] - 2, ptr(pred), stream()))
    return pred


def extract_features(ri, seg, feature_region=3, segments=8, sharp_num=4, less_sharp_num=8, flat_num=6):
    """a12 -> (feat f32 [B,H,W], key_point_map u8 [B,H,W])."""
    B, H, W = seg.shape
    feat = torch.empty((B, H, W), dtype=torch.float32, device=_dev(seg))
    kp = torch.empty((B, H, W), dtype=torch.uint8, device=_dev(seg))
    fn = _lib.lib().rpcc_extract_features_wide if seg.dtype == torch.uint16 else _lib.lib().rpcc_extract_features
    check(fn(ptr(ri), ptr(seg), B, H, W, feature_region, segments, sharp_num, less_sharp_num, flat_num, ptr(feat), ptr(kp), stream()))
    return feat, kp


def salience(seg, kp, level_kp_num, level_acc, ground_level, M):
    """a13 (levels) -> (salience u8 [B,K], label_acc f32 [B,K])."""
    B = seg.shape[0]
    P = seg[0].numel()
    K = M + 2
    L = len(level_kp_num)
    lk = (C.c_int32 * L)(*[int(x) for x in level_kp_num])
    la = (C.c_float * L)(*[float(x) for x in level_acc])
    sal = torch.empty((B, K), dtype=torch.uint8, device=_dev(seg))
    lacc = torch.empty((B, K), dtype=torch.float32, device=_dev(seg))
    check(_stage_entry("rpcc_salience", M, seg)(ptr(seg), ptr(kp), lk, la, L, int(ground_level), B, P, M, ptr(sal), ptr(lacc), stream()))
    return sal, lacc


def backproject(ri, tm):
    """a3: pc = ri[...,None] * transform_map -> f32 [B,H,W,3]."""
    B = ri.shape[0]
    P = ri[0].numel()
    pc = torch.empty(tuple(ri.shape[:3]) + (3,), dtype=torch.float32, device=_dev(ri))
    check(_lib.lib().rpcc_backproject(ptr(ri), ptr(tm), B, P, ptr(pc), stream()))
    return pc


def codec_workspace(B, P, M, device):
    """Work buffer of the contour codec and the decoder (cluster_num > 254: the wide decoder's sort buffers as well)."""
    n = _lib.lib().rpcc_wide_workspace_bytes(B, P, M, 0) if is_wide(M) else _lib.lib().rpcc_codec_workspace_bytes(B, P, M)
    return torch.empty(n, dtype=torch.uint8, device=device)


def contour_encode(seg, M=DEFAULT_CLUSTERS, ws=None):
    """f1: seg u8 [B,H,W] -> (contour_bits u8 [B,ceil(P/8)], idx_sequence u16 [B,P], nseq i32 [B])."""
    B, H, W = seg.shape
    P = H * W
    ws = codec_workspace(B, P, M, _dev(seg)) if ws is None else ws
    bits = torch.empty((B, (P + 7) // 8), dtype=torch.uint8, device=_dev(seg))
    seq = torch.empty((B, P), dtype=torch.uint16, device=_dev(seg))
    nseq = torch.empty((B,), dtype=torch.int32, device=_dev(seg))
    entry = _lib.lib().rpcc_contour_encode_wide if seg.dtype == torch.uint16 else _lib.lib().rpcc_contour_encode
    check(entry(ptr(seg), B, H, W, ptr(bits), ptr(seq), ptr(nseq), ptr(ws), stream()))
    return bits, seq, nseq


def contour_decode(bits, seq, H, W, M=DEFAULT_CLUSTERS, ws=None):
    """f3: recover_map on the packed contour bits -> seg u8 [B,H,W]."""
    B = bits.shape[0]
    P = H * W
    ws = codec_workspace(B, P, M, _dev(bits)) if ws is None else ws
    wide = is_wide(M)
    seg = torch.empty((B, H, W), dtype=torch.uint16 if wide else torch.uint8, device=_dev(bits))
    check((_lib.lib().rpcc_contour_decode_wide if wide else _lib.lib().rpcc_contour_decode)(ptr(bits), ptr(seq), B, H, W, ptr(seg), ptr(ws), stream()))
    return seg


def decode(seg, q16, model, tm, level_acc, salience=None, want_points=False, ws=None):
    """f3: dequantise + predict + reconstruct.  level_acc: float (uniform) or sequence (non-uniform, with
    salience u8 [B,K]).  -> (ri_rec f32 [B,H,W], pc_rec f32 [B,H,W,3] or None)."""
    B, H, W = seg.shape
    P = H * W
    M = model.shape[1] - 2
    ws = codec_workspace(B, P, M, _dev(seg)) if ws is None else ws
    uniform = salience is None
    acc = [float(level_acc)] if uniform else [float(a) for a in level_acc]
    arr = (C.c_double * len(acc))(*acc)
    rec = torch.empty((B, H, W), dtype=torch.float32, device=_dev(seg))
    pc = torch.empty((B, H, W, 3), dtype=torch.float32, device=_dev(seg)) if want_points else None
    entry = _lib.lib().rpcc_decode_wide if seg.dtype == torch.uint16 else _lib.lib().rpcc_decode
    check(entry(ptr(seg), ptr(q16), ptr(model), ptr(tm), arr, 0 if uniform else len(acc),
                ptr(salience), B, P, M, ptr(rec), ptr(pc), ptr(ws), stream()))
    return rec, pc


def decompress_workspace(B, P, M, device):
    """Work buffer of decompress_batch (rpcc_decompress_workspace_bytes; needs no initialisation)."""
    return torch.empty(max(_lib.lib().rpcc_decompress_workspace_bytes(B, P, M), 1), dtype=torch.uint8, device=device)


def decompress_batch(bits, seq, model, q16, payload_len, entropy_status, tm, level_acc, H, W, salience=None, want_points=True, ws=None, out=None):
    """f3 for a batch of streams (rpcc_decompress_batch; cluster_num above 254: rpcc_decompress_batch_wide): the decoded payloads of B frames as the
    entropy decoders left them -- bits u8 [B,ceil(P/8)], seq u16 [B,P], model f32 [B,K,4], q16 i16 [B,P], salience u8 [B,K] (non-uniform), every
    row padded to the geometry's maximum and free to hold anything past payload_len i64 [B,5] (container order; entropy_status i32 [B,5] likewise) --
    checked as tools/decompress.py:decode_frame checks them and decoded.  level_acc: float (uniform) or sequence (non-uniform, with salience).
    out: (status, seg, ri_rec, pc_rec or None) to write into.  -> (status i32 [B]: 0 or _lib.STREAM_E_*, seg [B,H,W], ri_rec f32 [B,H,W],
    pc_rec f32 [B,H,W,3] or None); a refused frame's rows are zero.  Nothing is waited for."""
    B, P, M = bits.shape[0], H * W, model.shape[1] - 2
    dev = _dev(bits)
    wide = is_wide(M)
    uniform = salience is None
    assert bits.shape == (B, (P + 7) // 8) and bits.dtype == torch.uint8 and seq.numel() == B * P and seq.dtype == torch.uint16
    assert q16.numel() == B * P and q16.dtype == torch.int16 and model.dtype == torch.float32 and model.shape == (B, M + 2, 4)
    assert payload_len.shape == (B, 5) and payload_len.dtype == torch.int64 and entropy_status.shape == (B, 5) and entropy_status.dtype == torch.int32
    assert uniform or (salience.shape == (B, M + 2) and salience.dtype == torch.uint8)
    acc = [float(level_acc)] if uniform else [float(a) for a in level_acc]
    arr = (C.c_double * len(acc))(*acc)
    ws = decompress_workspace(B, P, M, dev) if ws is None else ws
    if out is None:
        out = (torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B, H, W), dtype=label_dtype(M), device=dev),
               torch.empty((B, H, W), dtype=torch.float32, device=dev), torch.empty((B, H, W, 3), dtype=torch.float32, device=dev) if want_points else None)
    status, seg, rec, pc = out
    assert status.dtype == torch.int32 and status.numel() == B and seg.dtype == label_dtype(M) and seg.numel() == B * P
    assert rec.dtype == torch.float32 and rec.numel() == B * P and (pc is None or (pc.dtype == torch.float32 and pc.numel() == 3 * B * P))
    entry = _lib.lib().rpcc_decompress_batch_wide if wide else _lib.lib().rpcc_decompress_batch
    check(entry(ptr(bits), ptr(seq), ptr(model), ptr(q16), ptr(salience), ptr(payload_len), ptr(entropy_status), ptr(tm), arr, 0 if uniform else len(acc),
                B, H, W, M, ptr(status), ptr(seg), ptr(rec), ptr(pc), ptr(ws), stream()))
    return status, seg, rec, pc


def pack_payload(q16, nnz, packed=None, capacity=None, total=None):
    """f2: the batch's residual stream with the frames back to back (what the container / the payload gather holds):
    packed[:sum(nnz)] = concat_b q16[b][:nnz[b]].  `packed` (i16, >= capacity entries) and `total` (i64 [1]) are
    allocated when not given; capacity defaults to B*P.  -> (packed, total)."""
    B = q16.shape[0]
    P = q16.numel() // B
    if packed is None:
        packed = torch.zeros((B * P if capacity is None else int(capacity),), dtype=torch.int16, device=_dev(q16))
    capacity = packed.numel() if capacity is None else int(capacity)
    assert packed.numel() >= capacity and packed.dtype == torch.int16
    if total is None:
        total = torch.zeros((1,), dtype=torch.int64, device=_dev(q16))
    check(_lib.lib().rpcc_pack_payload(ptr(q16), ptr(nnz), B, P, ptr(packed), capacity, ptr(total), stream()))
    return packed, total


def check_cluster_num(M, wide=True, stage=None):
    """cluster_num as this build takes it.  The reference accepts any value (cfgs/compressor.yaml:22; its labels travel as uint16,
    utils/compress_utils.py:160).  Up to 254 the device keeps a pixel's label 0 .. cluster_num + 1 in ONE byte (the tuned kernels); above,
    the batch front-end (BatchBuffers / compress_batch / contour_encode / decode) takes the uint16 entries (rpcc_*_wide: the same results by
    plain kernels) up to 65 533.  wide=False: a caller that only has the byte-label stage entries (the mirror classes' per-stage calls) --
    a larger value is refused by name, before any buffer is allocated."""
    M = int(M)
    if stage == "mid":    # the uint16 stage entries (segmentation, point model, prediction, uniform quantiser): RPCC_MAX_CLUSTERS_MID
        if not 1 <= M <= _lib.MAX_CLUSTERS_MID:
            raise _lib.RpccError("cluster_num = %d: the stage-by-stage entries for segmentation, point model, prediction and the uniform quantiser support 1 <= "
                                 "cluster_num <= %d (their label tables live in LDS: RPCC_MAX_CLUSTERS_MID in include/rpcc_hip.h); pipeline.BatchCompressor "
                                 "takes up to 65533" % (M, _lib.MAX_CLUSTERS_MID))
        return M
    top = _lib.MAX_CLUSTERS_WIDE if wide else _lib.MAX_CLUSTERS
    if not 1 <= M <= top:
        raise _lib.RpccError("cluster_num = %d: %s supports 1 <= cluster_num <= %d (%s); the reference's default is 100 (cfgs/compressor.yaml:22)"
                             % (M, "this build" if wide else "the stage-by-stage entries", top,
                                "labels are uint16 in the container" if wide else
                                "their device labels are uint8: RPCC_MAX_CLUSTERS in include/rpcc_hip.h; pipeline.BatchCompressor takes up to 65533"))
    return M


def is_wide(M):
    return int(M) > _lib.MAX_CLUSTERS


class BatchBuffers:
    """Device buffers of one batch (B frames, one geometry), allocated once and reused.  general=True adds what the
    plane model / the non-uniform framework need (salience levels, key-point map, the larger work buffer)."""

    def __init__(self, B, geom, M, device, max_points=None, general=False, labels=False):
        """labels=True: the buffers of compress_batch_labels (the batch entered with a caller's label map) -- M is then its label cap
        (<= RPCC_MAX_CLUSTERS_MID), ws the work buffer of that entry (rpcc_labels_workspace_bytes: no projection, no FPS) and status
        i32 [B] its per-frame result.  Such buffers do not serve compress_batch."""
        M = check_cluster_num(M)
        self.wide = is_wide(M)     # uint16 labels, the rpcc_*_wide entries
        self.labels = bool(labels)
        self.labels_general = bool(general)
        if labels and M > _lib.MAX_CLUSTERS_MID:
            raise _lib.RpccError("label cap %d: compress_batch_labels takes labels up to RPCC_MAX_CLUSTERS_MID + 1 = %d (include/rpcc_hip.h)"
                                 % (M + 1, _lib.MAX_CLUSTERS_MID + 1))
        general = general or self.wide   # (the wide entry serves every framework / model combination from one workspace)
        P = geom.H * geom.W
        K = M + 2
        self.B, self.P, self.M, self.K, self.geom = B, P, M, K, geom
        f32, i32 = torch.float32, torch.int32
        self.ri = torch.empty((B, geom.H, geom.W), dtype=f32, device=device)
        self.seg = torch.empty((B, geom.H, geom.W), dtype=torch.uint16 if self.wide else torch.uint8, device=device)
        self.cen_pix = torch.empty((B, M), dtype=i32, device=device)
        self.centers = torch.empty((B, M, 3), dtype=f32, device=device)
        self.model = torch.empty((B, K, 4), dtype=f32, device=device)
        self.counts = torch.empty((B, K), dtype=i32, device=device)
        self.q16 = torch.empty((B, P), dtype=torch.int16, device=device)
        self.nnz = torch.empty((B,), dtype=i32, device=device)
        self.info = torch.empty((B, _lib.INFO_INTS), dtype=i32, device=device)
        # max_points: initial capacity (sum of N over the batch) of the projection's record space -- about 40 B of workspace per point
        # and 48 KB per frame (INTEGRATION.md "Memory").  Default one point per pixel: compress_batch re-allocates the workspace
        # when a batch holds more (dense or dual-return sweeps), so the default no longer reserves twice that up front.
        self.max_points = int(max_points) if max_points is not None else B * P
        self.general = bool(general)
        if labels:
            self.ws = labels_workspace(B, P, M, device, general=self.labels_general)
            self.status = torch.empty((B,), dtype=i32, device=device)
        else:
            self.ws = workspace(B, P, M, device, self.max_points, general=self.general)
        # (zeros, not empty: the library writes every level in the non-uniform framework and does not touch the tensor
        # in the uniform one, where consumers that copy it whole -- loader.StreamingCompressor's pinned copy, bench.py's
        # output dump -- then read defined bytes)
        self.salience = torch.zeros((B, K), dtype=torch.uint8, device=device) if general else None
        self.key_point_map = torch.empty((B, geom.H, geom.W), dtype=torch.uint8, device=device) if general else None


class FpsTimer:
    """rpcc_timer handle (bench.py): pass as compress_batch(timer=...) to time that call's FPS launch with HIP events."""

    def __init__(self):
        self.h = C.c_void_p(_lib.lib().rpcc_timer_create())
        assert self.h.value, "rpcc_timer_create failed"

    def reserve(self, launches):
        """Create the events of the next `launches` timed launches now (outside the caller's timed region)."""
        check(_lib.lib().rpcc_timer_reserve(self.h, int(launches)))

    def read(self):
        """-> (accumulated ms, launches) since the last read; synchronises the recorded events."""
        ms, n = C.c_double(0), C.c_int(0)
        check(_lib.lib().rpcc_timer_read(self.h, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def __del__(self):
        try:
            _lib.lib().rpcc_timer_destroy(self.h)
        except Exception:
            pass


def nonuniform_cfg(acc, cfg=None):
    """QuantizationModule's non-uniform settings (utils/compress_utils.py:36-54) as the C struct: acc = base step
    (2 * accuracy), cfg = compressor.yaml keys (level_key_point_num, level_delta_acc, ground_salience_level,
    feature_region, segments, sharp_num, less_sharp_num, flat_num)."""
    c = cfg or {}
    lk = list(c.get("level_key_point_num", (30, 10, 3, 0)))
    la = (np.array([acc] * len(lk)) + np.array(c.get("level_delta_acc", (0, 0.02, 0.04, 0.06)))).astype(np.float32)
    assert 1 <= len(lk) <= 8
    nu = _lib.NonuniformCfg()
    nu.levels = len(lk)
    for i, v in enumerate(lk):
        nu.level_kp_num[i] = int(v)
        nu.level_acc[i] = float(la[i])
    nu.ground_level = int(c.get("ground_salience_level", 2))
    nu.feature_region, nu.segments = int(c.get("feature_region", 3)), int(c.get("segments", 8))
    nu.sharp_num, nu.less_sharp_num, nu.flat_num = int(c.get("sharp_num", 4)), int(c.get("less_sharp_num", 8)), int(c.get("flat_num", 6))
    return nu


def compress_batch(xyz, offsets, tm, ground, buf, ground_threshold=0.1, acc=0.04, ground_seed=-1, frame_ids=None,
                   fps_bruteforce=False, timer=None, model_method="point", angle_threshold=75, plane_seed=0, nonuniform=None,
                   fps_fma=None, fps_cuda_tie=None, beams=None):
    """Fused a2..a13 for a batch, one call: FPS segmentation, point or plane model, uniform or non-uniform framework
    (tools/compress.py:93-125).  xyz: f32 [total,3], or the stored (x, y, z, intensity) rows f32 [total,4] (16-byte stride,
    no host-side slice).  ground f64 [B,4]: injected models when ground_seed < 0, otherwise output of the seeded
    ground RANSAC run inside the call (frame b draws with ground_seed + frame_ids[b]; frame_ids: stable identities,
    e.g. utils.frame_identity(path); default the batch position).  model_method "plane": rpcc_plane_model's seeded fits
    (plane_seed, frame_ids) with the reference's angle validation.  nonuniform: a nonuniform_cfg() struct -> key points,
    salience levels (buf.salience) and per-label steps; None = uniform framework with step `acc`.
    fps_fma / fps_cuda_tie: the CUDA-binary FPS modes (_lib.fps_mode_flags); None = the environment variables RPCC_FPS_FMA
    (0 / 1 / 2) and RPCC_FPS_TIE_CUDA, so every front-end (tools, pipeline, loader) honours them.
    beams (ops.beam_index of the lidar's per-beam elevation table; tm then is the ray table built from the same table): the projection
    stage goes through the table (rpcc_compress_batch_beams); cluster_num up to 1022."""
    io = _batch_io(xyz, offsets, tm, ground, buf, ground_seed, frame_ids, fps_bruteforce, timer, model_method, angle_threshold, plane_seed,
                   nonuniform, fps_fma, fps_cuda_tie)
    if beams is not None:
        _check_beams(beams, buf.geom)
        if buf.M > _lib.MAX_CLUSTERS_MID:
            raise NotImplementedError("cluster_num = %d with a per-beam elevation table: the table projection serves cluster_num <= %d "
                                      "(rpcc_compress_batch_beams)" % (buf.M, _lib.MAX_CLUSTERS_MID))
        buf._beams = beams            # (alive until the stream has consumed it)
        check(_lib.lib().rpcc_compress_batch_beams(C.byref(io), buf.B, buf.geom, ptr(beams), buf.M, float(ground_threshold), float(acc),
                                                   ptr(buf.ws), stream()))
        return buf
    entry = _lib.lib().rpcc_compress_batch_wide if buf.wide else _lib.lib().rpcc_compress_batch   # (cluster_num > 254: uint16 labels)
    check(entry(C.byref(io), buf.B, buf.geom, buf.M, float(ground_threshold), float(acc), ptr(buf.ws), stream()))
    return buf


def labels_workspace(B, P, M, device, general=False):
    """Work buffer of compress_batch_labels (rpcc_labels_workspace_bytes; needs no initialisation)."""
    n = _lib.lib().rpcc_labels_workspace_bytes(B, P, M, 1 if general else 0)
    if not n:
        raise _lib.RpccError("rpcc_labels_workspace_bytes(%d, %d, %d): no such batch (label cap 1 .. %d)" % (B, P, M, _lib.MAX_CLUSTERS_MID))
    return torch.empty((n + 255) // 256 * 256, dtype=torch.uint8, device=device)


def compress_batch_labels(ri, tm, ground, labels, max_label, buf, acc=0.04, model_method="point", angle_threshold=75, plane_seed=0,
                          frame_ids=None, nonuniform=None):
    """a8..a13 for a batch whose segmentation the caller has (rpcc_compress_batch_labels): ri f32 [B,H,W], ground f64 [B,4], labels i32
    [B,H,W] and max_label i32 [B] as dbscan.dbscan_segment returns them (ground 0, empty 1, noise 2, clusters from 3; -1 for a capped
    frame).  buf: BatchBuffers(B, geom, M, device, general=..., labels=True) with M the label CAP (labels up to M + 1); its seg, model,
    counts, q16, nnz (salience, key_point_map) are filled as compress_batch fills them.  -> buf.status i32 [B]: _lib.LABELS_OK, or
    _lib.LABELS_E_RANGE / _lib.LABELS_E_CAPPED for a refused frame, whose rows are zero bytes.  Nothing is waited for."""
    assert buf.labels, "BatchBuffers(..., labels=True) is needed"
    general = model_method != "point" or nonuniform is not None
    assert not general or buf.labels_general, "BatchBuffers(..., general=True) is needed for the plane model / non-uniform framework"
    B, P = buf.B, buf.P
    assert ri.dtype == torch.float32 and ri.numel() == B * P and labels.dtype == torch.int32 and labels.numel() == B * P
    assert max_label.dtype == torch.int32 and max_label.numel() == B and ground.dtype == torch.float64 and ground.numel() == 4 * B
    fid = _frame_ids(frame_ids, B, ri.device)
    buf._frame_ids, buf._nonuniform = fid, nonuniform   # (alive until the stream has consumed them)
    io = _lib.LabelsIO(ptr(ri).value, ptr(tm).value, ptr(ground).value, ptr(labels).value, ptr(max_label).value,
                       ptr(fid).value if fid is not None else None, ptr(buf.seg).value, ptr(buf.model).value, ptr(buf.counts).value,
                       ptr(buf.q16).value, ptr(buf.nnz).value, ptr(buf.status).value, 0 if model_method == "point" else 1,
                       angle_cos_cut(angle_threshold) if model_method != "point" else 0.0, int(plane_seed),
                       C.addressof(nonuniform) if nonuniform is not None else None,
                       ptr(buf.salience).value if nonuniform is not None else None,
                       ptr(buf.key_point_map).value if nonuniform is not None else None)
    check(_lib.lib().rpcc_compress_batch_labels(C.byref(io), B, buf.geom, buf.M, float(acc), ptr(buf.ws), stream()))
    return buf.status


STAGE_PROJECT, STAGE_GROUND, STAGE_MASK, STAGE_FPS, STAGE_LABELS, STAGE_PLANES, STAGE_QUANTISE = (1 << i for i in range(7))


def compress_batch_stages(stage_mask, xyz, offsets, tm, ground, buf, ground_threshold=0.1, acc=0.04, **kw):
    """The stages of compress_batch whose bits are set in stage_mask (STAGE_*), in order, on the current stream: for a caller that interleaves the
    stages of several batches on several streams (tools_dev/tick_bench.py).  Every stage needs its predecessors to have run on the same buffers."""
    assert not buf.wide
    io = _batch_io(xyz, offsets, tm, ground, buf, **kw)
    check(_lib.lib().rpcc_compress_batch_stages(C.byref(io), buf.B, buf.geom, buf.M, float(ground_threshold), float(acc), ptr(buf.ws), int(stage_mask), stream()))
    return buf


def _batch_io(xyz, offsets, tm, ground, buf, ground_seed=-1, frame_ids=None, fps_bruteforce=False, timer=None, model_method="point",
              angle_threshold=75, plane_seed=0, nonuniform=None, fps_fma=None, fps_cuda_tie=None):
    """The rpcc_batch_io of one geometry group (compress_batch's arguments); grows the group's workspace when the batch holds more points."""
    general = model_method != "point" or nonuniform is not None
    assert not general or buf.general, "BatchBuffers(..., general=True) is needed for the plane model / non-uniform framework"
    assert not buf.labels, "BatchBuffers(..., labels=True) serve compress_batch_labels only"
    if xyz.shape[0] > buf.max_points:
        buf.max_points = int(xyz.shape[0])
        buf.ws = workspace(buf.B, buf.P, buf.M, xyz.device, buf.max_points, general=buf.general)
    fid = _frame_ids(frame_ids, buf.B, xyz.device)
    buf._frame_ids = fid          # keep the tensor alive until the stream has consumed it
    buf._nonuniform = nonuniform  # (host struct read during the call only; kept for symmetry)
    return BatchIO(ptr(xyz).value, ptr(offsets).value, int(xyz.shape[0]), ptr(tm).value, ptr(ground).value,
                   int(ground_seed), ptr(fid).value if fid is not None else None, ptr(buf.ri).value, ptr(buf.seg).value,
                   ptr(buf.cen_pix).value, ptr(buf.centers).value, ptr(buf.model).value, ptr(buf.counts).value,
                   ptr(buf.q16).value, ptr(buf.nnz).value, ptr(buf.info).value,
                   (_lib.FPS_BRUTEFORCE if fps_bruteforce else 0) | _lib.fps_mode_flags(fps_fma, fps_cuda_tie),
                   timer.h if timer is not None else None,
                   0 if model_method == "point" else 1, angle_cos_cut(angle_threshold) if model_method != "point" else 0.0,
                   int(plane_seed), C.addressof(nonuniform) if nonuniform is not None else None,
                   ptr(buf.salience).value if nonuniform is not None else None,
                   ptr(buf.key_point_map).value if nonuniform is not None else None,
                   _point_stride(xyz))


def compress_batch_mixed(groups, ground_threshold=0.1, acc=0.04):
    """Fused a2..a13 for a batch that holds sweeps of several lidar geometries (variable H x W: BASELINE configs[4]), one call on the
    current stream.  groups: one dict per geometry with compress_batch's arguments (xyz, offsets, tm, ground, buf and, optionally,
    ground_seed, frame_ids, model_method, angle_threshold, plane_seed, nonuniform, fps_bruteforce, fps_fma, fps_cuda_tie); every buf is
    a BatchBuffers of that geometry with the same cluster count.  The kernels with one workgroup per frame or label (ground RANSAC,
    FPS, plane fits) run once over all groups (include/rpcc_hip.h: rpcc_compress_batch_mixed).  -> the list of the groups' buffers."""
    G = len(groups)
    assert 1 <= G <= _lib.MAX_GROUPS, "at most %d geometry groups per call" % _lib.MAX_GROUPS
    M = groups[0]["buf"].M
    assert all(g["buf"].M == M for g in groups), "one cluster count per call"
    if is_wide(M):   # (no mixed-geometry form of the uint16-label entry: the groups one after the other, same results)
        for g in groups:
            compress_batch(ground_threshold=ground_threshold, acc=acc, **g)
        return [g["buf"] for g in groups]
    ios = (BatchIO * G)(*[_batch_io(**g) for g in groups])
    Bs = (C.c_int * G)(*[g["buf"].B for g in groups])
    geoms = (_lib.Geom * G)(*[g["buf"].geom for g in groups])
    wss = (C.c_void_p * G)(*[ptr(g["buf"].ws).value for g in groups])
    check(_lib.lib().rpcc_compress_batch_mixed(ios, Bs, geoms, G, M, float(ground_threshold), float(acc), wss, stream()))
    return [g["buf"] for g in groups]


@functools.lru_cache(maxsize=64)
def angle_cos_cut(angle_threshold_deg):
    """Largest double v with arccos(v) > pi*(angle/180): the reference rejects a plane when
    alpha.max() > threshold (utils/segment_utils.py:89); the kernel compares v <= cos_cut instead of
    evaluating arccos per pixel.  Found by bisection on numpy's own arccos."""
    thr = np.pi * (angle_threshold_deg / 180)
    lo, hi = 0.0, 1.0          # arccos(lo) > thr >= arccos(hi)
    if not np.arccos(lo) > thr:
        return -1.0            # nothing in [0,1] is rejected
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if mid == lo or mid == hi:
            break
        if np.arccos(mid) > thr:
            lo = mid
        else:
            hi = mid
    return float(lo)


def plane_model(ri, tm, seg, M, angle_threshold=75, seed=0, ground=None, want_counts=False, frame_ids=None, inject=None, ws=None):
    """a9 -> model f32 [B,K,4] (and counts i32 [B,K]).  Label k of frame b draws with hash(seed, frame_ids[b], k).
    inject f64 [B,K,4] (test hook): planes used instead of the RANSAC results."""
    B = ri.shape[0]
    P = ri[0].numel()
    K = M + 2
    ws = torch.empty(_lib.lib().rpcc_plane_workspace_bytes(B, P, M), dtype=torch.uint8, device=_dev(ri)) if ws is None else ws
    model = torch.empty((B, K, 4), dtype=torch.float32, device=_dev(ri))
    counts = torch.empty((B, K), dtype=torch.int32, device=_dev(ri))
    fid = _frame_ids(frame_ids, B, _dev(ri))
    check(_stage_entry("rpcc_plane_model", M, seg)(ptr(ri), ptr(tm), ptr(seg), ptr(ground), B, P, M, angle_cos_cut(angle_threshold),
                                                   int(seed) & 0xFFFFFFFF, ptr(fid), ptr(inject), ptr(model), ptr(counts), ptr(ws), stream()))
    return (model, counts) if want_counts else model


def compress_batch_general(xyz, offsets, tm, ground, buf, cc, fit_ground, frame_ids=None):
    """Stage-by-stage batch path for the configurations the fused entry does not cover (non-uniform
    framework and / or plane model).  `cc` is a pipeline.BatchCompressor (settings holder).  Fills `buf`
    like compress_batch and returns the salience levels u8 [B,K] (None for the uniform framework)."""
    B, M, geom = buf.B, buf.M, buf.geom
    project(xyz, offsets, geom, ri=buf.ri)
    if fit_ground:
        g, _ = ground_ransac(buf.ri, tm, seed=cc.seed, frame_ids=frame_ids)
        ground.copy_(g)
    if _lib.fps_mode_flags(None, None):   # RPCC_FPS_FMA / RPCC_FPS_TIE_CUDA in the environment
        temp, info = ground_mask(buf.ri, tm, ground, cc.ground_threshold, fps_table=False)
        buf.info.copy_(info)
        _, centers = fps_range(buf.ri, tm, temp, info, M, cen_pix=buf.cen_pix, centers=buf.centers, fma=None, cuda_tie=None)
    else:
        temp, info, tab = ground_mask(buf.ri, tm, ground, cc.ground_threshold, fps_table=True)
        buf.info.copy_(info)
        _, centers = fps_range(buf.ri, tm, temp, info, M, fps_table=tab, cen_pix=buf.cen_pix, centers=buf.centers)
    assign(buf.ri, tm, ground, centers, out=buf.seg)
    if cc.model_method == "point":
        model, counts = point_model(buf.ri, buf.seg, ground, M, ws=buf.ws)
    else:
        model, counts = plane_model(buf.ri, tm, buf.seg, M, angle_threshold=cc.cfg.get("plane_angle_threshold", 75),
                                    seed=cc.seed, ground=ground, want_counts=True, frame_ids=frame_ids)
    buf.model.copy_(model)
    buf.counts.copy_(counts)
    sal = label_acc = None
    if not cc.uniform:
        c = cc.cfg
        _, kp = extract_features(buf.ri, buf.seg, c.get("feature_region", 3), c.get("segments", 8), c.get("sharp_num", 4),
                                 c.get("less_sharp_num", 8), c.get("flat_num", 6))
        lk = c.get("level_key_point_num", (30, 10, 3, 0))
        la = np.array([cc.acc] * len(lk)) + np.array(c.get("level_delta_acc", (0, 0.02, 0.04, 0.06)))
        sal, label_acc = salience(buf.seg, kp, lk, la.astype(np.float32), c.get("ground_salience_level", 2), M)
    predict_quantize(buf.ri, tm, buf.seg, buf.model, cc.acc, M, int16=True, ws=buf.ws, label_acc=label_acc,
                     q_out=buf.q16, nnz_out=buf.nnz)
    return sal
