"""Batched front-end: B frames of one lidar geometry through the fused HIP entry, then the host-side
payload assembly (casts, container, entropy coder) of the reference's compress_point_cloud /
save_compressed_bitstream.  This is the counterpart of the closure body of
tools/compress_datalist.py:91-142 for a whole batch at once.  BatchDecompressor is the way back: a list of .rpcc containers through one
entropy launch and one fused decode call per chunk.  What a container holds -- the columns, their order, dtypes and
bounds, and which part of a batch's buffers is one frame's -- is compress_utils.SCHEMA / columns / frame_slices."""
import numpy as np
import torch

from . import entropy, ops
from . import _lib
from .compress_utils import (BACKENDS, BEAM_TABLE_HIDDEN, BEAM_TABLE_INTENSITY, BEAM_TABLE_SUBPIXEL, HIDDEN_COLUMN, SCHEMA, TRAILERS, BasicCompressor, BatchPayload, columns, device_decoder,
                             frame_slices, intensity_trailer_span, pack_bitstream, pack_frames, payload_spans, unpack_bitstream)  # noqa: F401


class BatchCompressor:
    SLOTS = 4      # batches in flight one instance supports (submit() without collect()): every one owns its output buffers

    def __init__(self, transformer, cluster_num=100, accuracy=0.02, ground_threshold=0.1, uniform=True,
                 model_method="point", compressor_cfg=None, basic_compressor="bzip2", device=None, seed=0,
                 device_entropy=False, device_bzip2=False, segment_method="FPS", DBSCAN_eps=1.5, max_labels=None,
                 radius_outlier_removal=None, rans_delta=False, intensity_scale=None, point_format=None, subpixel_bits=None,
                 hidden_points=False):
        """point_format (None: float points, and nothing changes): "nclt" -- compress / submit take every frame as uint8 [N,8] NCLT
        velodyne_sync records (records.py); 8 bytes per point go up, records.unpack (librpcc_records.so) makes the stored rows on the
        device and run_batch reads them like any [N,4] rows, so every other option works behind it; with intensity_scale the payload
        is made of the records' intensity bytes (at scale 1 the byte itself).
        intensity_scale (None: off, and no byte of any container changes): frames are [N,>=4] rows (x, y, z, intensity); after the
        batch call one ops.intensity_encode runs on the same point tensor and the batch's range images, and every container gets the
        'intensity' trailer (compress_utils.pack_bitstream), byte for byte the per-frame path's.  Independent of the segmentation.
        subpixel_bits (None: off, and no byte of any container changes; else 1 .. 4): after the batch call one ops.subpixel_encode runs on
        the same point tensor and the batch's range images, and every container gets the 'subpixel' trailer behind the intensity one, byte
        for byte the per-frame path's.  Frames may be [N,3]: they get a zero fourth column on the host, the rows go up with stride 16.
        hidden_points (False: off, and no byte of any container changes): after the batch call one ops.hidden_encode runs on the same point
        tensor and the batch's range images -- step = accuracy * 2, lateral codes of subpixel_bits where that is set, else none -- and every
        container gets the 'hidden_points' trailer last, byte for byte the per-frame path's: the points that share a pixel with the one the
        range image keeps.  Frames may be [N,3], as for subpixel_bits.  The payload buffer is sized from the batch's largest frame.
        rans_delta (basic_compressor 'rans' only): the residual stream goes through the delta filter, as BasicCompressor(rans_delta=True)
        codes it on the per-frame path.
        segment_method "DBSCAN" (cfgs/compressor.yaml: segment_method, DBSCAN_eps): the frames are segmented by dbscan.dbscan_segment and
        enter the batch kernels through ops.compress_batch_labels; cluster_num does not apply (tools/compress.py).  max_labels: the labels a
        frame may use, 0 .. max_labels (default RPCC_MAX_CLUSTERS_MID + 1 = 1023, where the per-frame path raises too; up to 255: byte labels
        on the device); a frame with more makes collect() raise.
        radius_outlier_removal: None, or (nb_points, radius) -- the reference's use_radius_outlier_removal is (3, 1.0): every frame's points go
        through outlier.radius_outlier_mask first and the removed ones enter the projection as NaN, which it skips: the containers are those
        of the compacted frames, with no compaction, no new point count and no read-back in between."""
        from . import records
        self.point_format = records.check_point_format(point_format)
        self.outlier = None
        if radius_outlier_removal is not None:
            nb_points, radius = radius_outlier_removal
            if int(nb_points) < 0 or not float(radius) > 0:
                raise ValueError("radius_outlier_removal = %r: (nb_points >= 0, radius > 0)" % (radius_outlier_removal,))
            self.outlier = (int(nb_points), float(radius))
        if segment_method not in ("FPS", "DBSCAN"):
            raise ValueError("segment_method %r: FPS or DBSCAN" % (segment_method,))
        self.segment_method, self.eps = segment_method, float(DBSCAN_eps)
        if self.dbscan:
            top = _lib.MAX_CLUSTERS_MID + 1 if max_labels is None else int(max_labels)
            if not 2 <= top <= _lib.MAX_CLUSTERS_MID + 1:
                raise _lib.RpccError("max_labels = %d: the batch kernels take labels up to 2 .. RPCC_MAX_CLUSTERS_MID + 1 = %d (include/rpcc_hip.h)"
                                     % (top, _lib.MAX_CLUSTERS_MID + 1))
            self.M = top - 1          # the label cap of rpcc_compress_batch_labels: labels 0 .. M + 1
        else:
            self.M = ops.check_cluster_num(cluster_num)   # (above 254: uint16 labels through the rpcc_*_wide entries; above 65533: refused by name)
        self.T = transformer
        self.intensity_scale = None if intensity_scale is None else ops.check_intensity_scale(intensity_scale)
        if self.intensity_scale is not None and getattr(transformer, "even_dist", True) is False:
            raise NotImplementedError("BatchCompressor: " + BEAM_TABLE_INTENSITY)
        self.subpixel_bits = None if subpixel_bits is None else ops.check_subpixel_bits(subpixel_bits)
        if self.subpixel_bits is not None and getattr(transformer, "even_dist", True) is False:
            raise NotImplementedError("BatchCompressor: " + BEAM_TABLE_SUBPIXEL)
        self.hidden_points = bool(hidden_points)
        self.hidden_uncarried = None    # per frame of the last batch collected: hidden points the trailer does not carry
        self.hidden_carried = None      # ... and those it carries
        self.hidden_totals = [0, 0]     # carried, uncarried over every batch collected
        if self.hidden_points and getattr(transformer, "even_dist", True) is False:
            raise NotImplementedError("BatchCompressor: " + BEAM_TABLE_HIDDEN)
        # a transformer built from a per-beam elevation table (channel_distribute_csv): the projection goes through its index -- the fused
        # call's, the DBSCAN path's and the streaming loader's alike (all run_batch / _group_args); nothing behind the projection changes
        if getattr(transformer, "even_dist", True) is False and not self.dbscan and self.M > _lib.MAX_CLUSTERS_MID:
            raise NotImplementedError("cluster_num = %d with a per-beam elevation table (channel_distribute_csv): the table projection serves "
                                      "cluster_num <= %d" % (self.M, _lib.MAX_CLUSTERS_MID))
        self.device = torch.device(device) if device is not None else transformer.device
        self.acc = accuracy * 2                     # tools/compress.py:46
        self.ground_threshold = ground_threshold
        self.uniform = uniform
        self.model_method = model_method
        self.cfg = compressor_cfg or {}
        self.bc = BasicCompressor(method_name=basic_compressor, device_entropy=device_entropy, device_bzip2=device_bzip2,
                                  rans_delta=rans_delta)
        self.seed = int(seed)
        self._buf = None        # the buffers of the most recent call (tests read them after compress())
        self._codec_ws = None
        self._ring = {}         # frames per batch -> up to SLOTS BatchBuffers (+ codec workspace), busy between submit() and collect()

    @property
    def general(self):
        return not (self.uniform and self.model_method == "point")

    @property
    def beams(self):
        """The device index of the transformer's per-beam elevation table, or None (evenly spaced beams)."""
        return getattr(self.T, "beams_dev", None)

    @property
    def dbscan(self):
        return self.segment_method == "DBSCAN"

    def new_buffers(self, B, max_points=None):
        """The BatchBuffers run_batch fills for a batch of B frames (the streaming loader keeps one per slot)."""
        return ops.BatchBuffers(B, self.T.geom, self.M, self.device, max_points=max_points, general=self.general, labels=self.dbscan)

    def _filtered(self, xyz, offsets):
        """radius_outlier_removal: a copy of the points (packed xyz or the stored 16-byte rows alike) in which x, y, z of every removed point
        are NaN; without the option the points themselves, and nothing reaches librpcc_filter.so."""
        if self.outlier is None:
            return xyz
        from .outlier import radius_outlier_mask
        return radius_outlier_mask(xyz, offsets, self.outlier[0], self.outlier[1], masked=True).masked

    def run_intensity(self, rows, offsets, buf):
        """intensity_scale: the batch's intensity payloads into buf.intensity = (payload u8 [B, 8+P], nbytes i32 [B], orphans i32 [B]), on
        the current stream.  rows: the point tensor the range images in buf.ri were made of (the NaN-masked one with the radius filter)."""
        if self.intensity_scale is None:
            return
        if getattr(buf, "intensity", None) is None:
            B, P = buf.B, buf.P
            buf.intensity = (torch.empty((B, 8 + P), dtype=torch.uint8, device=self.device), torch.empty((B,), dtype=torch.int32, device=self.device),
                             torch.empty((B,), dtype=torch.int32, device=self.device))
            buf.intensity_scratch = torch.empty(_lib.lib().rpcc_intensity_scratch_bytes(B, P), dtype=torch.uint8, device=self.device)
        pay, nb, orphans = buf.intensity
        ops.intensity_encode(rows, offsets, self.T.geom, buf.ri, self.intensity_scale, payload=pay, nbytes=nb, orphans=orphans,
                             scratch=buf.intensity_scratch)

    def run_subpixel(self, rows, offsets, buf):
        """subpixel_bits: the batch's subpixel payloads into buf.subpixel = (payload u8 [B, 8+2P], nbytes i32 [B], orphans i32 [B]), on the
        current stream.  rows: the 16-byte rows the range images in buf.ri were made of (the NaN-masked ones with the radius filter)."""
        if self.subpixel_bits is None:
            return
        if getattr(buf, "subpixel", None) is None:
            B, P = buf.B, buf.P
            buf.subpixel = (torch.empty((B, 8 + 2 * P), dtype=torch.uint8, device=self.device), torch.empty((B,), dtype=torch.int32, device=self.device),
                            torch.empty((B,), dtype=torch.int32, device=self.device))
            buf.subpixel_scratch = torch.empty(_lib.lib().rpcc_subpixel_scratch_bytes(B, P), dtype=torch.uint8, device=self.device)
        pay, nb, orphans = buf.subpixel
        ops.subpixel_encode(rows, offsets, self.T.geom, buf.ri, self.subpixel_bits, payload=pay, nbytes=nb, orphans=orphans,
                            scratch=buf.subpixel_scratch)

    def run_hidden(self, rows, offsets, buf, max_rows=None):
        """hidden_points: the batch's hidden_points payloads into buf.hidden = (payload u8 [B, 16 + P + 4 max_rows], nbytes i32 [B], orphans
        i32 [B], uncarried i32 [B]), on the current stream.  rows: the 16-byte rows the range images in buf.ri were made of (the NaN-masked
        ones with the radius filter).  max_rows: the rows of the batch's largest frame (None: no frame has more rows than the batch)."""
        if not self.hidden_points:
            return
        B, P, total = buf.B, buf.P, int(rows.shape[0])
        width = ops.hidden_row_bytes(P, total if max_rows is None else max_rows)
        if getattr(buf, "hidden", None) is None or buf.hidden[0].shape[1] < width:
            buf.hidden = (torch.empty((B, width), dtype=torch.uint8, device=self.device),) + tuple(
                torch.empty((B,), dtype=torch.int32, device=self.device) for _ in range(3))
        need = _lib.lib().rpcc_hidden_scratch_bytes(B, P, total)
        if getattr(buf, "hidden_scratch", None) is None or buf.hidden_scratch.numel() < need:
            buf.hidden_scratch = torch.empty(need, dtype=torch.uint8, device=self.device)
        pay, nb, orphans, uncarried = buf.hidden
        ops.hidden_encode(rows, offsets, self.T.geom, buf.ri, self.acc, self.subpixel_bits or 0, payload=pay, nbytes=nb, orphans=orphans,
                          uncarried=uncarried, scratch=buf.hidden_scratch)

    def run_trailers(self, rows, offsets, buf, max_rows=None):
        """The optional channels behind the batch call, in container order.  max_rows: run_hidden's."""
        self.run_intensity(rows, offsets, buf)
        self.run_subpixel(rows, offsets, buf)
        self.run_hidden(rows, offsets, buf, max_rows)

    @staticmethod
    def check_orphans(orphans, channel="intensity"):
        if np.any(orphans):
            raise _lib.RpccError("%s: frames %s have non-empty pixels no row owns (the range image is not the image of these rows)"
                                 % (channel, np.flatnonzero(orphans).tolist()))

    def check_hidden(self, nbytes, orphans, uncarried, heads):
        """A batch's hidden_points lengths, orphan and uncarried counts and the payload rows' bytes 12 .. 15 (m) on the host: raises for
        orphans and for a payload row that was too short (nbytes -1: the buffer was not sized from the batch's largest frame); keeps the
        batch's uncarried and carried counts per frame in self.hidden_uncarried / self.hidden_carried and adds them to self.hidden_totals."""
        self.check_orphans(orphans, "hidden_points")
        if np.any(np.asarray(nbytes) < 0):
            raise _lib.RpccError("hidden_points: the payload rows of frames %s are too short for their points" % np.flatnonzero(np.asarray(nbytes) < 0).tolist())
        self.hidden_uncarried = np.asarray(uncarried).copy()
        self.hidden_carried = np.ascontiguousarray(heads).view("<u4").reshape(-1).astype(np.int64)
        self.hidden_totals[0] += int(self.hidden_carried.sum())
        self.hidden_totals[1] += int(self.hidden_uncarried.sum())

    def run_batch(self, xyz, offsets, ground, buf, frame_ids=None, fit_ground=True, max_rows=None):
        """The device work of one batch into buf, on the current stream, nothing waited for.  max_rows (hidden_points): the rows of the
        batch's largest frame, which size the payload rows; None: the batch's row count, which no frame exceeds.  ground f64 [B,4]: fitted here (fit_ground: the
        seeded RANSAC, frame b drawing with seed + frame_ids[b]) or the caller's.  FPS: one ops.compress_batch.  DBSCAN: ops.project (packed
        xyz or the stored 16-byte rows), ops.ground_ransac with the per-frame path's seed and identities, dbscan_segment(min_points = 10,
        as the reference hard-codes it) without the read-back of its max_label, then ops.compress_batch_labels, whose per-frame status
        (buf.status) collect() reads."""
        nu = None if self.uniform else ops.nonuniform_cfg(self.acc, self.cfg)
        angle = self.cfg.get("plane_angle_threshold", 75)
        xyz = self._filtered(xyz, offsets)
        if not self.dbscan:
            ops.compress_batch(xyz, offsets, self.T.tm_dev, ground, buf, self.ground_threshold, self.acc,
                               ground_seed=self.seed if fit_ground else -1, frame_ids=frame_ids, model_method=self.model_method,
                               angle_threshold=angle, plane_seed=self.seed, nonuniform=nu, beams=self.beams)
            self.run_trailers(xyz, offsets, buf, max_rows)
            return
        from .dbscan import dbscan_segment
        tm = self.T.tm_dev
        ops.project(xyz, offsets, self.T.geom, ri=buf.ri, beams=self.beams)
        if fit_ground:
            g, _ = ops.ground_ransac(buf.ri, tm, seed=self.seed, frame_ids=frame_ids)
            ground.copy_(g)
        labels, top = dbscan_segment(buf.ri, tm, ground, self.eps, min_points=10, check=False)
        ops.compress_batch_labels(buf.ri, tm, ground, labels, top, buf, self.acc, model_method=self.model_method, angle_threshold=angle,
                                  plane_seed=self.seed, frame_ids=frame_ids, nonuniform=nu)
        self.run_trailers(xyz, offsets, buf, max_rows)

    def check_status(self, status):
        """status: a batch's buf.status on the host (None for FPS).  Raises RpccError naming the refused frames (their places in the batch)
        and the label limit, in the words of PointCloudSegment._dbscan and dbscan_segment."""
        if status is None or not np.any(status):
            return
        bad = [int(i) for i in np.flatnonzero(status)]
        capped = [int(i) for i in np.flatnonzero(np.asarray(status) == _lib.LABELS_E_CAPPED)]
        if capped:
            raise _lib.RpccError("librpcc_seg: a union-find loop hit its iteration cap (frames %s)" % (capped,))
        raise _lib.RpccError("DBSCAN found labels above %d in frames %s: the batch kernels take labels up to max_labels = %d (at most "
                             "RPCC_MAX_CLUSTERS_MID + 1 = %d, include/rpcc_hip.h); use a larger DBSCAN_eps"
                             % (self.M + 1, bad, self.M + 1, _lib.MAX_CLUSTERS_MID + 1))

    def _buffers(self, B):
        """Output buffers for a batch of B frames: the first set no submit() holds (collect() reads a batch's counts, models, salience and
        contour bits from them, so a second submit() before the first collect() must not land in the same set); at most SLOTS sets per
        batch size, created when first needed.  compress_device() alone never holds a set: its results are valid until the next call."""
        ring = self._ring.setdefault(B, [])
        buf = next((b for b in ring if not b.in_flight), None)
        if buf is None:
            if len(ring) >= self.SLOTS:
                raise RuntimeError("BatchCompressor: %d batches submitted and not collected; collect() one before the next submit()" % len(ring))
            buf = self.new_buffers(B)
            buf.codec_ws = ops.codec_workspace(B, self.T.H * self.T.W, self.M, self.device)
            buf.in_flight = False
            ring.append(buf)
        self._buf, self._codec_ws = buf, buf.codec_ws
        return buf

    def _group_args(self, xyz, offsets, ground=None, frame_ids=None):
        """ops.compress_batch's arguments for this compressor's settings (one geometry group of ops.compress_batch_mixed)."""
        B = offsets.numel() - 1
        buf = self._buffers(B)
        fit = ground is None
        g = torch.zeros((B, 4), dtype=torch.float64, device=self.device) if fit else ground
        # one fused call for all four framework / model combinations (tools/compress.py:109-124)
        nu = None if self.uniform else ops.nonuniform_cfg(self.acc, self.cfg)
        args = dict(xyz=xyz, offsets=offsets, tm=self.T.tm_dev, ground=g, buf=buf, ground_seed=self.seed if fit else -1, frame_ids=frame_ids,
                    model_method=self.model_method, angle_threshold=self.cfg.get("plane_angle_threshold", 75), plane_seed=self.seed, nonuniform=nu)
        if self.beams is not None:   # (never inside a mixed-geometry call: MixedBatchCompressor refuses such transformers)
            args["beams"] = self.beams
        return args

    def _encode(self, args):
        """Contour bits / index sequences of the segmentation a fused call left in args["buf"]."""
        buf = args["buf"]
        sal = None if self.uniform else buf.salience
        bits, seq, nseq = ops.contour_encode(buf.seg, self.M, ws=buf.codec_ws)
        return buf, args["ground"], bits, seq, nseq, sal

    def compress_device(self, xyz, offsets, ground=None, frame_ids=None, max_rows=None):
        """Device part.  xyz f32 [sum N,3], offsets i64 [B+1] on the device.  Returns the BatchBuffers plus
        contour bits / index sequences (and salience for the non-uniform framework), all still in HBM.
        frame_ids: stable identities of the frames (utils.frame_identity) for the seeded plane fits.  max_rows: run_batch's."""
        if self.dbscan:
            buf = self._buffers(offsets.numel() - 1)
            g = torch.zeros((buf.B, 4), dtype=torch.float64, device=self.device) if ground is None else ground
            self.run_batch(xyz, offsets, g, buf, frame_ids, fit_ground=ground is None, max_rows=max_rows)
            return self._encode(dict(buf=buf, ground=g))
        args = self._group_args(self._filtered(xyz, offsets), offsets, ground, frame_ids)
        ops.compress_batch(ground_threshold=self.ground_threshold, acc=self.acc, **args)
        self.run_trailers(args["xyz"], offsets, args["buf"], max_rows)
        return self._encode(args)

    def _upload(self, frames, ground=None):
        """Host arrays of a batch -> device (xyz, offsets, ground or None) on the current stream."""
        if self.point_format == "nclt":
            return self._upload_records(frames, ground)
        offs = np.zeros(len(frames) + 1, np.int64)
        offs[1:] = np.cumsum([f.shape[0] for f in frames])
        cols = 3 if self.intensity_scale is None else 4     # (with intensity the rows go up as stored: the kernels read them with stride 16)
        if cols == 4 and any(f.ndim != 2 or f.shape[1] < 4 for f in frames):
            raise ValueError("BatchCompressor(intensity_scale=...): frames must be [N,>=4] rows (x, y, z, intensity)")
        if cols == 3 and (self.subpixel_bits is not None or self.hidden_points):     # the owner pass reads 16-byte rows: xyz and a zero fourth column where a frame has none
            from .compress_utils import rows16
            frames, cols = [rows16(f) for f in frames], 4
        xyz = torch.from_numpy(np.ascontiguousarray(np.concatenate([f[:, :cols] for f in frames]), dtype=np.float32)).to(self.device)
        gnd = None if ground is None else torch.from_numpy(np.asarray(ground, np.float64).reshape(-1, 4)).to(self.device)
        return xyz, torch.from_numpy(offs).to(self.device), gnd, int(offs[-1])

    def _upload_records(self, frames, ground=None):
        """point_format "nclt": the frames' records go up as they are, 8 bytes per point, and records.unpack writes the stored rows
        on the current stream -> what _upload returns, the rows [sum N,4] in the place of xyz."""
        from . import records
        recs = [records.as_records(f) for f in frames]
        offs = np.zeros(len(recs) + 1, np.int64)
        offs[1:] = np.cumsum([r.shape[0] for r in recs])
        host = np.concatenate(recs) if recs else np.zeros((0, records.RECORD_BYTES), np.uint8)
        with torch.cuda.device(self.device):
            rows = records.unpack(torch.from_numpy(host).to(self.device))
        gnd = None if ground is None else torch.from_numpy(np.asarray(ground, np.float64).reshape(-1, 4)).to(self.device)
        return rows, torch.from_numpy(offs).to(self.device), gnd, int(offs[-1])

    def _payload(self, n, npts, xyz, dev_out):
        """The two variable-length 16-bit streams leave the device with the frames back to back (rpcc_pack_payload), not as the padded
        [B,P] arrays: nnz <= points of the frame, one index per contour start <= pixels.  -> the context collect() takes."""
        buf, g, bits, seq, nseq, sal = dev_out
        qp, qtot = ops.pack_payload(buf.q16, buf.nnz, capacity=npts)
        sp, stot = ops.pack_payload(seq.view(torch.int16), nseq)
        buf.in_flight = True    # until collect() has read it (_buffers)
        # the batch's buffer of every column (compress_utils.SCHEMA; frame_slices cuts the frames out of them) and the per-frame counts
        pay, nbytes, _ = buf.intensity if self.intensity_scale is not None else (None, None, None)
        spay, nsub, _ = buf.subpixel if self.subpixel_bits is not None else (None, None, None)
        hpay, nhid, _, _ = buf.hidden if self.hidden_points else (None, None, None, None)
        bufs = dict(salience_level=sal, contour_map=bits, idx_sequence=sp, plane_param=buf.model, residual_quantized=qp, intensity=pay, subpixel=spay,
                    hidden_points=hpay)
        ctx = dict(n=n, buf=buf, bufs=bufs, counts=(buf.counts, buf.nnz, nseq, nbytes, nsub, nhid), tot=dict(nnz=qtot, nseq=stot),
                   stream=torch.cuda.current_stream(self.device), keep=(xyz, g, seq))
        codec = self.bc.batch_codec()
        if codec:
            ctx["containers"] = self._device_containers(codec[0], bufs, *ctx["counts"])
        return ctx

    @property
    def columns(self):
        return columns(self.uniform, self.intensity_scale is not None, self.subpixel_bits is not None, self.hidden_points)

    def _device_containers(self, codec, bufs, counts, nnz, nseq, nbytes, nsub=None, nhid=None):
        """basic_compressor 'lz4' without the lz4 package (codec: lz4_codec), 'deflate' / 'gzip' with device_entropy (deflate_codec),
        'bzip2' with device_bzip2 (bzip2_codec) or 'rans' (rans_codec, a typed back-end: it is also told each column's element width, as
        the per-frame path takes it from the arrays' itemsize, and -- with rans_delta -- each column's filter, by the same rule from its
        dtype): the batch's .rpcc containers are built in HBM (the codec's encode_descriptors over the arrays where they lie -- the
        columns' bounds and dtypes from compress_utils.SCHEMA, their places from frame_slices -- then rpcc_lz4_pack_containers, which
        asks nothing of the streams' format) on the current stream.  -> (containers, frame offsets / lengths)."""
        from . import lz4_codec
        (B, K), P, cols = counts.shape, self.T.H * self.T.W, self.columns
        at = frame_slices(cols, bufs, counts, nnz, nseq, nbytes, nsub, nhid)
        # per frame, in container order: device address and bytes of every column
        addr = torch.stack([bufs[c.name].data_ptr() + c.dtype.itemsize * at[c.name][0] for c in cols], 1).reshape(-1)
        lens = torch.stack([c.dtype.itemsize * at[c.name][1] for c in cols], 1).reshape(-1)
        typed = BACKENDS[self.bc.method_name].typed
        kw = dict(widths=[c.dtype.itemsize for c in cols] * B) if typed else {}
        if typed and self.bc.rans_delta:      # delta for the residual column only (rans_codec.delta_filter)
            kw["filters"] = [codec.delta_filter(c.dtype) for c in cols] * B
        # (the hidden_points column's bound is its buffer's row: 16 + P + 4 rows of the batch's largest frame)
        bounds = [int(bufs[c.name].shape[1]) if c.cut == "nhid" else c.bound(P, K) for c in cols]
        slots, dst_off, dst_len, _ = codec.encode_descriptors(addr, lens, bounds * B, **kw)
        cap = int(slots.numel()) + 4 * len(cols) * B
        out, frame = lz4_codec.pack_containers(slots, dst_off, dst_len, B, len(cols), cap)
        return out, frame, (addr, lens, slots, dst_off, dst_len)

    def submit(self, frames, ground=None, frame_ids=None):
        """Device part of compress() on the current stream, nothing waited for.  -> a context for collect()."""
        xyz, offs, gnd, npts = self._upload(frames, ground)
        max_rows = None
        if self.hidden_points:      # the payload rows are sized from the batch's largest frame
            from . import records
            max_rows = max(((records.as_records(f) if self.point_format == "nclt" else f).shape[0] for f in frames), default=0)
        return self._payload(len(frames), npts, xyz, self.compress_device(xyz, offs, gnd, frame_ids, max_rows=max_rows))

    def collect(self, ctx, pool=None):
        """Waits for submit()'s stream and assembles the .rpcc byte strings (host part: casts, container, entropy coder).
        pool: a concurrent.futures executor -- the frames' entropy coding then runs on its threads (bz2 / zlib / lz4
        release the GIL), like the reference's --workers ThreadPoolExecutor (tools/compress_datalist.py:202-206)."""
        buf, built = ctx["buf"], ctx.get("containers")
        try:
            ctx["stream"].synchronize()
            if built:       # by _device_containers: the frames' places now, the containers in one copy below
                fr = built[1].cpu().numpy()
            else:           # the columns' buffers, the packed ones as far as the batch filled them
                bufs, tot, cols = ctx["bufs"], ctx["tot"], self.columns
                counts, nnz, nseq, nbytes, nsub, nhid = (None if t is None else t.cpu().numpy() for t in ctx["counts"])
                host = {c.name: (bufs[c.name][: int(tot[c.cut].item())] if c.cut in tot else bufs[c.name]).cpu().numpy() for c in cols}
            status = buf.status.cpu().numpy() if self.dbscan else None
            orphans = buf.intensity[2].cpu().numpy() if self.intensity_scale is not None else None
            sub_orphans = buf.subpixel[2].cpu().numpy() if self.subpixel_bits is not None else None
            hid = tuple(t.cpu().numpy() for t in buf.hidden[1:] + (buf.hidden[0][:, 12:16],)) if self.hidden_points else None
        finally:
            buf.in_flight = False   # everything collect() needs is on the host -- or the call failed: either way the slot is free again
        n = ctx["n"]
        self.check_status(status)
        if orphans is not None:
            self.check_orphans(orphans[:n])
        if sub_orphans is not None:
            self.check_orphans(sub_orphans[:n], "subpixel")
        if hid is not None:
            self.check_hidden(*(h[:n] for h in hid))
        if built:
            if (fr[1, :n] < 0).any():
                raise RuntimeError("rpcc_lz4: the containers of frames %s were not built" % np.flatnonzero(fr[1, :n] < 0).tolist())
            h = built[0][: int((fr[0, :n] + fr[1, :n]).max()) if n else 0].cpu().numpy()
            return [h[o: o + l].tobytes() for o, l in zip(fr[0, :n], fr[1, :n])]
        assemble = BatchPayload(cols, host, counts, nnz, nseq, nbytes, nsub=nsub, nhid=nhid).frame      # the object the streaming loader assembles from
        # a few frames per task: one call into the host library per chunk (compress_utils.pack_frames)
        step = max(1, n // 64) if pool is not None else max(n, 1)
        chunk = lambda lo: pack_frames(self.bc, [assemble(b) for b in range(lo, min(lo + step, n))], uniform=self.uniform)
        parts = list(pool.map(chunk, range(0, n, step))) if pool is not None else [chunk(lo) for lo in range(0, n, step)]
        return [blob for part in parts for blob in part]

    def discard(self, ctx):
        """Gives up a submit() whose results are not wanted (a caller that aborts a batch): waits for its stream -- the kernels may still
        be writing the slot -- and frees the slot.  Without it (or collect()) the slot stays busy and the ring runs out after SLOTS such calls."""
        try:
            ctx["stream"].synchronize()
        finally:
            ctx["buf"].in_flight = False

    def compress(self, frames, ground=None, pool=None, frame_ids=None):
        """frames: list of [N,3] arrays.  -> list of .rpcc byte strings (one per frame)."""
        return self.collect(self.submit(frames, ground, frame_ids), pool=pool)


class MixedBatchCompressor:
    """BASELINE configs[4]: one batch holding sweeps of several lidar geometries (variable H x W).  The frames are grouped by
    geometry and the groups go through ONE fused call (ops.compress_batch_mixed / rpcc_compress_batch_mixed): the kernels with one
    workgroup per frame or per label -- ground RANSAC, FPS, plane fits: latency-bound whatever the image size -- run once over all
    groups, the pixel-parallel ones group after group; the results come back in input order.  (Until round 4 every group ran as its
    own chain of launches on its own stream: the device runs three or four kernels side by side, so three chains of small
    launches left most of it idle -- profiles/HISTORY.md.)
    transformers: {lidar name: PCTransformer}; the other arguments are BatchCompressor's."""

    SLOTS = BatchCompressor.SLOTS   # mixed batches in flight of the streaming form (submit / collect on SLOTS streams): every lidar's compressor
                                    # keeps that many buffer sets, a further submit() before a collect() raises

    def __init__(self, transformers, **kw):
        if kw.get("segment_method", "FPS") != "FPS":
            raise NotImplementedError("MixedBatchCompressor: segment_method %r -- the mixed-geometry call runs FPS only; DBSCAN: one "
                                      "BatchCompressor(segment_method='DBSCAN') per lidar" % (kw["segment_method"],))
        if kw.get("intensity_scale") is not None:
            raise NotImplementedError("MixedBatchCompressor: intensity_scale -- the mixed-geometry call carries no intensity; use one "
                                      "BatchCompressor(intensity_scale=...) per lidar")
        if kw.get("subpixel_bits") is not None:
            raise NotImplementedError("MixedBatchCompressor: subpixel_bits -- the mixed-geometry call carries no subpixel offsets; use one "
                                      "BatchCompressor(subpixel_bits=...) per lidar")
        if kw.get("hidden_points"):
            raise NotImplementedError("MixedBatchCompressor: hidden_points -- the mixed-geometry call carries no hidden points; use one "
                                      "BatchCompressor(hidden_points=True) per lidar")
        if kw.get("radius_outlier_removal") is not None:
            raise NotImplementedError("MixedBatchCompressor: radius_outlier_removal -- the mixed-geometry call takes the points as they are; "
                                      "filter them first (outlier.radius_outlier_mask), or use one BatchCompressor per lidar")
        if kw.get("point_format") is not None:
            raise NotImplementedError("MixedBatchCompressor: point_format %r -- the mixed-geometry call takes float points; unpack the "
                                      "records first (records.unpack), or use one BatchCompressor(point_format=...) per lidar" % (kw["point_format"],))
        tabled = sorted(name for name, t in transformers.items() if getattr(t, "even_dist", True) is False)
        if tabled:
            raise NotImplementedError("MixedBatchCompressor: lidars %s have a per-beam elevation table (channel_distribute_csv) -- the "
                                      "mixed-geometry call projects evenly spaced beams only; use one BatchCompressor per such lidar" % (tabled,))
        self.bcs = {name: BatchCompressor(t, **kw) for name, t in transformers.items()}
        first = next(iter(self.bcs.values()))
        self.device, self.ground_threshold, self.acc = first.device, first.ground_threshold, first.acc

    def compress_device(self, parts):
        """parts: {lidar name: (xyz, offsets, ground or None, frame_ids or None)} on the device.  One fused call on the current stream
        -> {lidar name: what BatchCompressor.compress_device returns}."""
        args = {name: self.bcs[name]._group_args(*part) for name, part in parts.items()}
        ops.compress_batch_mixed(list(args.values()), ground_threshold=self.ground_threshold, acc=self.acc)
        return {name: self.bcs[name]._encode(a) for name, a in args.items()}

    def submit(self, frames, lidars):
        """Device part of compress() on the current stream, nothing waited for.  -> a context for collect()."""
        groups = {}
        for i, name in enumerate(lidars):
            groups.setdefault(name, []).append(i)
        up = {name: self.bcs[name]._upload([frames[i] for i in idx]) for name, idx in groups.items()}
        outs = self.compress_device({name: (xyz, offs, gnd, None) for name, (xyz, offs, gnd, _) in up.items()})
        ctxs = {name: self.bcs[name]._payload(len(groups[name]), up[name][3], up[name][0], outs[name]) for name in groups}
        return dict(n=len(frames), groups=groups, ctxs=ctxs)

    def collect(self, ctx, pool=None):
        out = [None] * ctx["n"]
        for name, idx in ctx["groups"].items():
            for i, blob in zip(idx, self.bcs[name].collect(ctx["ctxs"][name], pool=pool)):
                out[i] = blob
        return out

    def compress(self, frames, lidars):
        """frames: list of [N,3] arrays; lidars: the lidar name of every frame.  -> list of .rpcc byte strings."""
        return self.collect(self.submit(frames, lidars))


STREAM_TEXT = {_lib.STREAM_E_ENTROPY: "an entropy stream was refused by the device decoder",
               _lib.STREAM_E_PLANE: "plane_param payload is not a whole number of float32 [.,4] rows, or holds more than cluster_num + 2 rows",
               _lib.STREAM_E_CONTOUR: "contour_map does not hold the bytes this range image needs (wrong --lidar?)",
               _lib.STREAM_E_WIDTH: "idx_sequence / residual_quantized payloads are not 16-bit arrays",
               _lib.STREAM_E_NSEQ: "idx_sequence does not hold one label per run the contour map marks",
               _lib.STREAM_E_LABEL: "idx_sequence names a label without a stored model row",
               _lib.STREAM_E_SALIENCE: "salience_level does not fit the model rows or the configured levels",
               _lib.STREAM_E_RESIDUAL: "residual_quantized does not hold one value per non-empty pixel of the label map",
               _lib.STREAM_E_CONTAINER: "the container's length prefixes do not fit its bytes",
               _lib.STREAM_E_INTENSITY: "no valid intensity payload follows the geometry (compressed without intensity, or the payload does not fit the label map; a "
                                        "container that also carries the subpixel trailer gives its intensity on the per-frame path only)",
               _lib.STREAM_E_SUBPIXEL: "no valid subpixel payload follows the geometry where the trailers asked for place it (compressed without --subpixel, or "
                                       "the payload does not fit the label map or holds a code past its bits)",
               _lib.STREAM_E_HIDDEN: "no valid hidden_points payload follows the geometry where the trailers asked for place it (compressed without "
                                     "--hidden_points, or the payload does not fit the label map, or it holds more points than hidden_capacity)"}


def container_spans(blob, uniform=True):
    """The (offset, length) of every payload of one .rpcc container by unpack_bitstream's rules (compress_utils), in container order; None for
    a container they refuse: a prefix that is cut off or negative, or a payload longer than the bytes left."""
    spans = list(payload_spans(blob, len(columns(uniform))))
    return spans if len(spans) == len(columns(uniform)) else None


class BatchDecompressor:
    """The .rpcc containers of FPS streams (cluster_num fixed by the configuration) decoded a chunk at a time: the containers' length prefixes are
    parsed on the host, the chunk's bytes go up in one copy, ONE launch of the back-end's device decoder writes every stream of the chunk
    straight into the padded [B, ...] arrays rpcc_decompress_batch reads -- what a stream may decode to follows from the geometry alone -- and
    one ops.decompress_batch checks and decodes the frames (status per frame: _lib.STREAM_E_*).  A lidar with a per-beam elevation table
    (PCTransformer(cfg, channel_distribute_csv)) needs nothing of its own here: the decoder reads the transformer's ray table -- built from that
    table -- and nothing else of the geometry, so streams of such a lidar decode with the transformer they were encoded with.
    accuracy / level_acc / uniform are
    tools/decompress.py:decode_frame's arguments, and its results are this class's, bit for bit.  The device decoders are used whatever the
    device_entropy / device_bunzip2 flags of a BasicCompressor handed in say: those govern the per-frame path.
    DBSCAN streams size their label count per frame (cluster_num=None, as decode_frame takes it): with max_labels=N they are decoded under the
    label cap N - 1 -- rpcc_decompress_batch takes a frame's row count from its plane payload -- with decode_frame(..., None, ...)'s refusals; a
    frame with more rows than the cap is decoded once more through decode_frame.  Label maps come back in the cap's dtype.
    device_trailers=True (opt-in) decodes the subpixel and hidden_points trailers here as well; without it the two
    are refused by name and every result is what it was before the flag existed."""

    CHUNK_FRAMES = 32              # frames per chunk at most, as the datalist tool reads them
    CHUNK_BUDGET_BYTES = 2 << 30   # device bytes one chunk may take: padded payloads, bzip2 work slots, work buffer and outputs

    def __init__(self, transformer, cluster_num, accuracy, uniform=True, level_acc=None, basic_compressor="bzip2", max_labels=None,
                 intensity=False, subpixel=False, hidden_points=False, device_trailers=False, hidden_capacity=None):
        """intensity=True: every container must carry the 'intensity' trailer (BatchCompressor(intensity_scale=...), --intensity):
        decompress_device returns a fifth tensor, f32 [B,H,W], decompress 4-tuples; a frame without a valid trailer gets
        _lib.STREAM_E_INTENSITY (unless an earlier status applies) and a zero row.  The scale is read from each payload's header.
        device_trailers=True: subpixel=True and hidden_points=True are taken too, alone, together and with intensity.  What follows a
        container's geometry must then be exactly the trailers asked for, in file order, ending the blob (unpack_bitstream's rule).
        subpixel: pc_rec holds the turned points.  hidden_points: decompress_device also returns (hidden f32 [B,cap,3], hidden_count i32 [B])
        last, decompress returns points [P + m, 3]; hidden_capacity (None: P) is the cap, the hidden points per frame this path holds -- a
        frame with more comes back through decode_frame like any E_HIDDEN frame, so no sound container fails because of it.  A frame's
        status is the first that is not OK of: its geometry status (E_ENTROPY when one of its trailers' streams was refused by the entropy
        decoder), E_INTENSITY, E_SUBPIXEL, E_HIDDEN; a refused frame's images are zeros and its hidden count is 0."""
        self.device_trailers = bool(device_trailers)
        if subpixel and not self.device_trailers:
            raise NotImplementedError("BatchDecompressor: subpixel -- the batch decoder back-projects along the pixels' centre rays; decode "
                                      "containers with the subpixel trailer per frame (tools.decompress.decode_frame(..., subpixel=True)), or "
                                      "pass device_trailers=True")
        if hidden_points and not self.device_trailers:
            raise NotImplementedError("BatchDecompressor: hidden_points -- the batch decoder returns one point per pixel; decode containers "
                                      "with the hidden_points trailer per frame (tools.decompress.decode_frame(..., hidden_points=True)), or "
                                      "pass device_trailers=True")
        self.intensity, self.subpixel, self.hidden_points = bool(intensity), bool(subpixel), bool(hidden_points)
        if self.subpixel:
            transformer.subpixel_tables()     # (a per-beam elevation table: NotImplementedError, as on the per-frame path)
        self.per_frame_rows = cluster_num is None     # DBSCAN streams
        if cluster_num is None:
            if max_labels is None:
                raise ValueError("BatchDecompressor: cluster_num=None (a DBSCAN stream sizes its label count per frame) needs max_labels, the "
                                 "label cap of the batch (1023 at most); or decode such streams with tools.decompress.decode_frame")
            if not 2 <= int(max_labels) <= _lib.MAX_CLUSTERS_MID + 1:
                raise _lib.RpccError("max_labels = %d: 2 .. RPCC_MAX_CLUSTERS_MID + 1 = %d" % (int(max_labels), _lib.MAX_CLUSTERS_MID + 1))
            cluster_num = int(max_labels) - 1
        self.cluster_num = None if self.per_frame_rows else cluster_num   # what decode_frame is given
        self.M = ops.check_cluster_num(cluster_num)
        self.T, self.device = transformer, transformer.device
        self.accuracy, self.uniform = accuracy, bool(uniform)
        if not self.uniform and level_acc is None:
            raise ValueError("BatchDecompressor: the non-uniform framework needs level_acc")
        self.level_acc = None if level_acc is None else [float(a) for a in level_acc]
        self.method = basic_compressor.method_name if isinstance(basic_compressor, BasicCompressor) else basic_compressor
        assert self.method in BasicCompressor.METHODS, "Compression method is not existed. (lz4, bzip2, gzip, deflate, rans)"
        self.host_bc = BasicCompressor(method_name=self.method)   # the E_ENTROPY fallback: the host library's decoder
        self.work_bytes, self.decode_slots = device_decoder(self.method)   # the device decoder, whatever the flags say
        P, K = transformer.H * transformer.W, self.M + 2
        # the geometry's columns (compress_utils.SCHEMA) and the decoded bytes a stream of each can have: fixed by the geometry; the trailer's alike
        self.cols = columns(self.uniform)
        self.ns = len(self.cols)
        self.caps = [c.bound(P, K) for c in self.cols]
        self.trailer_cap = columns(self.uniform, True)[-1].bound(P, K)
        self.hidden_capacity = (P if hidden_capacity is None else int(hidden_capacity)) if self.hidden_points else 0
        if self.hidden_capacity < 0:
            raise ValueError("BatchDecompressor: hidden_capacity %d" % self.hidden_capacity)
        # the trailers asked for, in file order, and the decoded bytes a stream of each can have: 8 + P, 8 + 2P, 16 + P + 4 hidden_capacity
        self.trailers = tuple(t for t, on in zip(TRAILERS, (self.intensity, self.subpixel, self.hidden_points)) if on)
        self.trailer_caps = {"intensity": self.trailer_cap, "subpixel": SCHEMA[6].bound(P, K), "hidden_points": HIDDEN_COLUMN.bound(P, K, self.hidden_capacity)}
        self.chunk = max(1, min(self.CHUNK_FRAMES, self.CHUNK_BUDGET_BYTES // self._frame_bytes()))

    def _frame_bytes(self):
        """Device bytes a frame of a chunk takes at most (bzip2: every stream at level 9)."""
        P, t = self.T.H * self.T.W, self.trailer_cap
        work = sum(self.work_bytes(b"BZh9", c) for c in self.caps)
        outs = P * (2 if ops.is_wide(self.M) else 1) + 4 * P + 12 * P
        ws = -(-_lib.lib().rpcc_decompress_workspace_bytes(self.CHUNK_FRAMES, P, self.M) // self.CHUNK_FRAMES)
        inten = (2 * t + 4 * P + self.work_bytes(b"BZh9", t)) if self.intensity else 0   # coded + decoded trailer, the f32 image, its work slot
        # the other trailers alike (the subpixel points are pc_rec's); the hidden points [cap,3] and their count
        more = sum(2 * c + self.work_bytes(b"BZh9", c) for c in (self.trailer_caps[t] for t in self.trailers if t != "intensity"))
        more += (12 * self.hidden_capacity + 4) if self.hidden_points else 0
        return sum(self.caps) + 5 * 256 + work + outs + ws + inten + more

    def _descriptors(self, m, addr, lens, dst_off, dst_cap, heads):
        """The six descriptor rows decode_slots takes, [addr | lens | dst_off | dst_cap | work_off | work_cap], into m (host i64 [6, n]): the
        work slots -- 8-byte multiples, 0 where the decoder takes none -- sized from each stream's first bytes and packed back to back.
        -> the work buffer's bytes."""
        m[0], m[1], m[2], m[3] = addr, lens, dst_off, dst_cap
        m[5] = [self.work_bytes(h, c) for h, c in zip(heads, m[3].tolist())]
        m[4], wtotal = entropy.packed_slots(m[5])
        return wtotal

    def _chunk_device(self, blobs, out, data=None):
        """One chunk: parse, upload, entropy launch, decode call on the current stream.  out: the chunk's rows of (status, seg, rec, pc).
        data: (device u8 tensor, offsets) when the containers are on the device already (the tensor must stay alive until the stream has run)."""
        B, ns, dev = len(blobs), self.ns, self.device
        H, W, K = self.T.H, self.T.W, self.M + 2
        spans = [container_spans(b, self.uniform) for b in blobs]
        sound = [i for i, sp in enumerate(spans) if sp is not None]
        n = ns * len(sound)
        # the padded arrays, one allocation: a part per column of self.cols, B rows of the column's bound, every part 256-aligned
        row = self.caps
        part = np.zeros(ns + 1, np.int64)
        part[1:] = np.cumsum([(B * r + 255) // 256 * 256 for r in row])
        arrays = [entropy.as_bytes(b) for b in blobs]
        boff, bend = entropy.aligned_slots([a.size for a in arrays])
        # descriptors [addr | lens | dst_off | dst_cap | work_off | work_cap | sound frames | refused frames] and the chunk's bytes: one pinned buffer
        nmeta = 6 * n + B
        host = torch.empty(8 * nmeta + ((bend + 7) // 8 * 8 if data is None else 0), dtype=torch.uint8, pin_memory=True)
        up = torch.empty(host.numel(), dtype=torch.uint8, device=dev)
        meta_h = host[: 8 * nmeta].numpy().view(np.int64)
        base = up.data_ptr() + 8 * nmeta if data is None else data[0].data_ptr()
        offs = boff if data is None else data[1]
        if data is None:
            body = host[8 * nmeta:].numpy()
            for a, o in zip(arrays, boff):
                body[o: o + a.size] = a
        sp = np.array([spans[i] for i in sound], np.int64).reshape(len(sound), ns, 2)
        fr = np.array(sound, np.int64)
        wtotal = self._descriptors(meta_h[: 6 * n].reshape(6, n), (base + offs[fr][:, None] + sp[:, :, 0]).reshape(-1), sp[:, :, 1].reshape(-1),
                                   (part[None, :ns] + fr[:, None] * np.array(row, np.int64)[None, :]).reshape(-1), np.tile(np.array(row, np.int64), len(sound)),
                                   [arrays[i][o: o + min(l, 4)] for i in sound for o, l in spans[i]])
        work = torch.empty(wtotal, dtype=torch.uint8, device=dev) if wtotal else None
        bad = np.array([i for i in range(B) if spans[i] is None], np.int64)
        meta_h[6 * n: 6 * n + len(sound)], meta_h[6 * n + len(sound): 6 * n + B] = fr, bad
        up.copy_(host, non_blocking=True)
        meta = up[: 8 * nmeta].view(torch.int64)
        d = [meta[k * n: (k + 1) * n] for k in range(6)]
        dst = torch.empty(int(part[-1]), dtype=torch.uint8, device=dev)
        dst_len, est = self.decode_slots(d, dst, work)
        # [B,5] lengths / statuses in container order (uniform: no salience column); a frame whose container was refused: status 1, no length
        plen = torch.zeros((B, 5), dtype=torch.int64, device=dev)
        pest = torch.ones((B, 5), dtype=torch.int32, device=dev)
        if len(sound) == B:
            plen[:, 5 - ns:], pest[:, 5 - ns:] = dst_len.view(B, ns), est.view(B, ns)
        elif sound:
            idx = meta[6 * n: 6 * n + len(sound)]
            plen[idx, 5 - ns:], pest[idx, 5 - ns:] = dst_len.view(-1, ns), est.view(-1, ns)
        # the parts as [B, ...] arrays of their columns' dtypes; the last four in file order are decompress_batch's first four arguments
        typed = [dst[int(part[i]): int(part[i]) + B * row[i]].view(getattr(torch, c.dtype.name)).view(B, -1) for i, c in enumerate(self.cols)]
        bits, seq, model, q16 = typed[-4:]
        # (subpixel: no centre-ray points -- ops.subpixel_decode writes the turned ones into out[3] below)
        ops.decompress_batch(bits, seq, model.view(B, K, 4), q16, plen, pest, self.T.tm_dev, self.accuracy if self.uniform else self.level_acc,
                             H, W, salience=None if self.uniform else typed[0], out=out[:3] + (None,) if self.subpixel else out[:4])
        if len(bad):
            out[0][meta[6 * n + len(sound): 6 * n + B]] = _lib.STREAM_E_CONTAINER
        if self.per_frame_rows and not self.uniform:
            # decode_frame(..., None, ...) sizes K from the frame: max(rows, 3).  A salience payload longer than that is refused there, although it
            # fits the cap's K -- ahead of the residual check, behind all others (rpcc_decompress_batch's order)
            st = out[0]
            late = ((st == _lib.STREAM_OK) | (st == _lib.STREAM_E_RESIDUAL)) & (plen[:, 0] > torch.clamp(plen[:, 3] // 16, min=3))
            st.masked_fill_(late, _lib.STREAM_E_SALIENCE)
            for o in out[1:]:
                if o is not None:   # a refused frame's rows are zero (uint16 label maps: through their int16 view)
                    (o.view(torch.int16) if o.dtype == torch.uint16 else o).masked_fill_(late.view((B,) + (1,) * (o.dim() - 1)), 0)
        if self.trailers:
            self._chunk_trailers(blobs, arrays, base, offs, out)

    def _trailer_spans(self, blob):
        """(start, length) of the coded bytes of every trailer asked for, in file order, or None.  device_trailers: unpack_bitstream's rule --
        what follows the geometry is exactly these trailers, ending the blob.  Without it: intensity_trailer_span's one-trailer rule."""
        if not self.device_trailers:
            sp = intensity_trailer_span(blob, self.uniform)
            return None if sp is None else [(sp[0], sp[1] - sp[0])]
        tail, nt = list(payload_spans(blob, self.ns + len(TRAILERS)))[self.ns:], len(self.trailers)
        return tail[:nt] if len(tail) >= nt and sum(tail[nt - 1]) == len(blob) else None

    def _tables(self, needed):
        """The device copy of the subpixel tables; None where a hidden_points decoder has none to give (a per-beam elevation table: a frame
        with lateral codes is then refused, E_HIDDEN, and decode_frame says why)."""
        try:
            return self.T.subpixel_tables()
        except NotImplementedError:
            if needed:
                raise
            return None

    def _chunk_trailers(self, blobs, arrays, base, offs, out):
        """The chunk's wanted trailers: one more decode_slots call writes every one of them into a padded [B, bound] array of its own, then
        ops.intensity_decode / ops.subpixel_decode / ops.hidden_decode run on the label maps and ranges just decoded.  Without
        device_trailers (intensity alone): a frame without a (valid) trailer, or whose geometry was refused, keeps its earlier status or
        gets STREAM_E_INTENSITY, and a zero row.  With it: a frame's status is the first that is not OK of geometry (E_ENTROPY when the
        entropy decoder refused one of its trailers), E_INTENSITY, E_SUBPIXEL, E_HIDDEN, and a refused frame's outputs are all zeros."""
        B, dev, want, nt = len(blobs), self.device, self.trailers, len(self.trailers)
        row = np.array([self.trailer_caps[t] for t in want], np.int64)
        part = np.zeros(nt + 1, np.int64)
        part[1:] = np.cumsum((B * row + 255) // 256 * 256)       # a part per trailer, B rows of its bound, every part 256-aligned
        spans = [self._trailer_spans(b) for b in blobs]
        have = [i for i, sp in enumerate(spans) if sp is not None]
        n = len(have)
        nbytes = torch.zeros((nt, B), dtype=torch.int32, device=dev)     # 0: no trailer, refused by the payload decoders
        refused = torch.zeros((B,), dtype=torch.bool, device=dev)        # a trailer's stream the entropy decoder refused
        pay = torch.empty(int(part[-1]), dtype=torch.uint8, device=dev)
        if n:
            fr = np.array(have, np.int64)
            sp = np.array([spans[i] for i in have], np.int64).reshape(n, nt, 2)
            meta_h = torch.empty((7, n * nt), dtype=torch.int64, pin_memory=True)
            m = meta_h.numpy()
            wtotal = self._descriptors(m, (base + offs[fr][:, None] + sp[:, :, 0]).reshape(-1), sp[:, :, 1].reshape(-1),
                                       (part[None, :nt] + fr[:, None] * row[None, :]).reshape(-1), np.tile(row, n),
                                       [arrays[i][s: s + min(l, 4)] for i in have for s, l in spans[i]])
            m[6] = np.repeat(fr, nt)
            meta = meta_h.to(dev, non_blocking=True)
            work = torch.empty(wtotal, dtype=torch.uint8, device=dev) if wtotal else None
            dst_len, est = self.decode_slots([meta[k] for k in range(6)], pay, work)
            ok, idx = (est == 0).view(n, nt), meta[6].view(n, nt)[:, 0]
            nbytes[:, idx] = torch.where(ok, dst_len.view(n, nt), torch.zeros_like(dst_len.view(n, nt))).to(torch.int32).t()
            if self.device_trailers:
                refused[idx] = ~ok.all(1)
        rows = {t: pay[int(part[k]): int(part[k]) + B * int(row[k])].view(B, int(row[k])) for k, t in enumerate(want)}
        nb = {t: nbytes[k] for k, t in enumerate(want)}
        status, seg, rec = out[:3]
        if not self.device_trailers:
            inten = out[4]
            _, ist = ops.intensity_decode(rows["intensity"], nb["intensity"], seg, out=inten)
            bad = status != _lib.STREAM_OK
            inten.masked_fill_(bad.view(B, 1, 1), 0)
            status.copy_(torch.where(bad, status, ist))
            return
        st = torch.where((status == _lib.STREAM_OK) & refused, torch.full_like(status, _lib.STREAM_E_ENTROPY), status)
        outs = [seg, rec]
        if self.intensity:
            _, tst = ops.intensity_decode(rows["intensity"], nb["intensity"], seg, out=out[4])
            st = torch.where(st != _lib.STREAM_OK, st, tst)
            outs.append(out[4])
        if self.subpixel:    # (a caller that wants no points still wants the payload's verdict, as decode_frame gives it)
            pc = out[3] if out[3] is not None else torch.empty((B,) + tuple(rec.shape[1:]) + (3,), dtype=torch.float32, device=dev)
            _, tst = ops.subpixel_decode(rows["subpixel"], nb["subpixel"], seg, rec, self._tables(True), out=pc)
            st = torch.where(st != _lib.STREAM_OK, st, tst)
        if out[3] is not None:
            outs.append(out[3])
        if self.hidden_points:
            hid, count = out[-2], out[-1]
            _, _, tst = ops.hidden_decode(rows["hidden_points"], nb["hidden_points"], seg, self.T.tm_dev, self._tables(False), out=hid, count=count)
            st = torch.where(st != _lib.STREAM_OK, st, tst)
            outs.append(count)
        status.copy_(st)
        bad = st != _lib.STREAM_OK
        for o in outs:      # a refused frame's rows are zero (uint16 label maps: through their int16 view)
            (o.view(torch.int16) if o.dtype == torch.uint16 else o).masked_fill_(bad.view((B,) + (1,) * (o.dim() - 1)), 0)

    def upload(self, blobs):
        """The containers' bytes on the device, a chunk per copy, for decompress_device(blobs, uploaded=...): callers that hold the containers
        in HBM already (the length prefixes are still read from the host copies)."""
        with torch.cuda.device(self.device):
            return [entropy.upload([entropy.as_bytes(b) for b in blobs[c0: c0 + self.chunk]], self.device) for c0 in range(0, len(blobs), self.chunk)]

    def decompress_device(self, blobs, want_points=True, uploaded=None):
        """blobs: .rpcc byte strings of one geometry and configuration (uploaded: what upload(blobs) returned, else they are copied up here).  -> (status i32 [B]: 0 or _lib.STREAM_E_*, seg [B,H,W], ri_rec f32 [B,H,W],
        pc_rec f32 [B,H,W,3] or None) GPU tensors, queued on the current stream and not waited for; a refused frame's rows are zero."""
        B, H, W, dev = len(blobs), self.T.H, self.T.W, self.device
        out = (torch.empty((B,), dtype=torch.int32, device=dev), torch.empty((B, H, W), dtype=ops.label_dtype(self.M), device=dev),
               torch.empty((B, H, W), dtype=torch.float32, device=dev), torch.empty((B, H, W, 3), dtype=torch.float32, device=dev) if want_points else None)
        if self.intensity:
            out += (torch.empty((B, H, W), dtype=torch.float32, device=dev),)
        if self.hidden_points:
            out += (torch.empty((B, self.hidden_capacity, 3), dtype=torch.float32, device=dev), torch.empty((B,), dtype=torch.int32, device=dev))
        with torch.cuda.device(dev):
            for c0 in range(0, B, self.chunk):
                c1 = min(c0 + self.chunk, B)
                self._chunk_device(blobs[c0: c1], tuple(None if o is None else o[c0: c1] for o in out), None if uploaded is None else uploaded[c0 // self.chunk])
        return out

    def rows_buffers(self, n):
        """The device buffers one chunk of at most n frames is decoded into on its way to rows: decompress_device's outputs, chunk-sized."""
        H, W, dev = self.T.H, self.T.W, self.device
        out = (torch.empty((n,), dtype=torch.int32, device=dev), torch.empty((n, H, W), dtype=ops.label_dtype(self.M), device=dev),
               torch.empty((n, H, W), dtype=torch.float32, device=dev), torch.empty((n, H, W, 3), dtype=torch.float32, device=dev))
        out += (torch.empty((n, H, W), dtype=torch.float32, device=dev),) if self.intensity else ()
        return out + ((torch.empty((n, self.hidden_capacity, 3), dtype=torch.float32, device=dev), torch.empty((n,), dtype=torch.int32, device=dev))
                      if self.hidden_points else ())

    def decompress_rows_device(self, blobs, uploaded=None, images=None):
        """The .bin rows of the batch instead of its images (rows.py, librpcc_rows.so).  -> (status i32 [B], offsets i64 [B+1], rows f32 [B*H*W,4],
        nonzero i32 [B]) GPU tensors, queued on the current stream and not waited for: frame b is rows[offsets[b]:offsets[b+1]], the frames back
        to back (a refused frame has no rows), nonzero[b] its pixels with a range != 0; with intensity=True the fourth column is the decoded
        intensity, else +0.0.  Each chunk is decoded into the same chunk-sized images (images: rows_buffers(self.chunk) of the caller's, else
        allocated here) and packed behind the chunk before: no image of the batch exists, here or on the host."""
        from . import cloud, rows as R
        B, P, dev = len(blobs), self.T.H * self.T.W, self.device
        status = torch.empty((B,), dtype=torch.int32, device=dev)
        offsets = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
        out_rows = torch.empty((B * (P + self.hidden_capacity), 4), dtype=torch.float32, device=dev)   # (hidden_points: cloud.pack, the hidden points behind the image's)
        nonzero = torch.empty((B,), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            images = self.rows_buffers(min(self.chunk, B)) if images is None and B else images
            base = None
            for c0 in range(0, B, self.chunk):
                n = min(self.chunk, B - c0)
                out = tuple(o[:n] for o in images)
                self._chunk_device(blobs[c0: c0 + n], out, None if uploaded is None else uploaded[c0 // self.chunk])
                if self.hidden_points:
                    table, _, _ = cloud.pack(out[3], out[4] if self.intensity else None, out[2], extra=out[-2], extra_count=out[-1], rows=out_rows,
                                             nonzero=nonzero[c0: c0 + n], base=base)
                else:
                    table, _, _ = R.pack(out[3], out[4] if self.intensity else None, out[2], rows=out_rows, nonzero=nonzero[c0: c0 + n], base=base)
                status[c0: c0 + n] = out[0]
                offsets[c0: c0 + n + 1] = table[: n + 1]
                base = table[n: n + 1]
        return status, offsets, out_rows, nonzero

    def rows_fallback(self, blob, index):
        """A frame the device decoder refused with a status decompress() falls back on: once more through decode_frame with the host library,
        its rows by the numpy rule.  -> (rows f32 [n,4], nonzero).  Any other status, and what the host library refuses too: ValueError."""
        from . import rows as R
        from .tools.decompress import decode_frame, point_intensity
        flags = dict(intensity=self.intensity, subpixel=self.subpixel, hidden_points=self.hidden_points)
        try:
            rec, pc, _, *w = decode_frame(unpack_bitstream(blob, self.uniform, **flags), self.host_bc, self.T, self.cluster_num,
                                          self.accuracy, self.level_acc, self.uniform, **flags)
        except (ValueError, OSError, EOFError) as e:
            raise ValueError("frame %d: %s" % (index, e)) from e
        return R.pack_host(pc, (point_intensity(w[0], pc) if self.hidden_points else w[0]) if w else None), int((rec != 0).sum())

    def falls_back(self, st):
        """decompress()'s rule: E_ENTROPY, E_PLANE on a DBSCAN stream (more rows than the cap) and E_HIDDEN (more points than hidden_capacity
        on a sound payload; what is damaged the per-frame path refuses in words) go through the per-frame path."""
        return st == _lib.STREAM_E_ENTROPY or (st == _lib.STREAM_E_PLANE and self.per_frame_rows) or st == _lib.STREAM_E_HIDDEN

    def refusal(self, st, index):
        return ValueError("frame %d: %s (status %d)" % (index, STREAM_TEXT.get(int(st), "refused"), int(st)))

    def decompress_rows(self, blobs):
        """-> [float32 [n_b,4] host arrays]: the rows tools/decompress_datalist.py writes to <name>.bin, byte for byte.  Per chunk only status,
        offsets and rows[:total] cross the link (a caller that wants the point counts too takes them from decompress_rows_device).  The fallback and the errors are decompress()'s."""
        res = []
        for c0 in range(0, len(blobs), self.chunk):
            part = blobs[c0: c0 + self.chunk]
            status, offsets, rows, _ = self.decompress_rows_device(part)
            status, offsets = status.cpu().numpy(), offsets.cpu().numpy()
            host = rows[: int(offsets[-1])].cpu().numpy()
            for i, st in enumerate(status):
                if st == _lib.STREAM_OK:
                    res.append(host[offsets[i]: offsets[i + 1]])
                elif self.falls_back(st):
                    res.append(self.rows_fallback(part[i], c0 + i)[0])
                else:
                    raise self.refusal(st, c0 + i)
        return res

    def decompress(self, blobs, want_points=True):
        """-> [(rec f32 [H,W], pc f32 [H,W,3] or None, seg [H,W])] as tools/decompress.py:decode_frame returns them, a chunk's arrays in one
        copy each.  A frame whose entropy streams the device decoder refuses (E_ENTROPY: bzip2 with trailing bytes or the randomised bit, a
        second gzip member, the empty blob -- or a damaged stream) is decoded once more through decode_frame with the host library, which
        raises for what it refuses too; any other refusal raises ValueError with the frame's index and the status text."""
        from .tools.decompress import decode_frame
        res = []
        for c0 in range(0, len(blobs), self.chunk):
            part = blobs[c0: c0 + self.chunk]
            flags = dict(intensity=self.intensity, subpixel=self.subpixel, hidden_points=self.hidden_points)
            status, seg, rec, pc, *w = (None if t is None else t.cpu().numpy() for t in self.decompress_device(part, want_points))
            for i, st in enumerate(status):
                if st == _lib.STREAM_OK:
                    pts = pc[i] if pc is not None else None
                    if self.hidden_points and pts is not None:     # decode_frame's [P + m, 3]: the image points, then the hidden points
                        pts = np.concatenate([pts.reshape(-1, 3), w[-2][i, : int(w[-1][i])]])
                    res.append((rec[i], pts, seg[i]) + ((w[0][i],) if self.intensity else ()))
                    continue
                if not self.falls_back(st):   # (more rows than the cap, more hidden points than the cap: per frame)
                    raise ValueError("frame %d: %s (status %d)" % (c0 + i, STREAM_TEXT.get(int(st), "refused"), int(st)))
                try:
                    res.append(decode_frame(unpack_bitstream(part[i], self.uniform, **flags), self.host_bc, self.T, self.cluster_num,
                                            self.accuracy, self.level_acc, self.uniform, want_points=want_points, **flags))
                except (ValueError, OSError, EOFError) as e:
                    raise ValueError("frame %d: %s" % (c0 + i, e)) from e
        return res
