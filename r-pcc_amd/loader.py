"""f4: the input pipeline that keeps the kernels fed -- counterpart of the reference's datalist loop
(tools/compress_datalist.py:91-142,202-206: a thread pool whose workers each load, compress and write one file).

The device part runs at > 10^5 frames/s; a frame is 1.36 MB of points, so the feed is bounded by the host copy into
pinned memory and by the PCIe link (52 GB/s measured = 38.7 k frames/s of 64x2048), not by the kernels.  StreamingCompressor
therefore overlaps the three parts for consecutive batches:

    pool threads   read / copy the frames of batch n+1 straight into a PINNED staging slot (no intermediate concatenation)
    copy stream    slot -> device buffer of batch n+1 (non_blocking H2D), event
    compute stream waits for that event, rpcc_compress_batch + contour codec + payload packing of batch n, D2H of the
                   packed payload into pinned output buffers, event
    pool threads   entropy coding + container + file output of batch n-1 (optional)

submit(n+1) -- with the default depth of 4 also submit(n+2) -- is issued before collect(n), so the copy engine always has a
staged batch waiting.  Slots (staging, device input, BatchBuffers, output) form a ring of `depth`.

StreamingDecompressor is the way back: .rpcc files in, .bin files out, a chunk per stream with up to `depth` chunks in flight; only the
files' bytes (rows.pack on the device) and a few words per frame come back, and the pool reads and writes files meanwhile.
"""
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

from . import _lib, ops, pointfile, records
from .compress_utils import BatchPayload, pack_bitstream, pack_frames  # noqa: F401
from .utils import available_cpus


class _Slot:
    def __init__(self, bc, B, cap_points, device, cols=3, nclt=False, fields=False):
        P, K = bc.T.H * bc.T.W, bc.M + 2
        self.B, self.cap, self.cols = B, int(cap_points), int(cols)    # cols: floats per point in the staging / device input (3 or 4)
        self.nclt = bool(nclt)      # ingest="nclt": records are staged and sent (8 bytes per point); xyz_dev [cap,4] is filled on the device
        self.fields = bool(fields)  # ingest="fields": the .pcd / .ply files' bytes are staged and sent; xyz_dev [cap,4] is filled on the device
        self.cap_bytes, self.nbytes = 32 * self.cap, 0     # (fields) bytes of the chunk buffers -- a sizing hint, grow_bytes -- and of the staged chunk
        self._point_buffers(device)
        self.offs_pin = torch.zeros((B + 1,), dtype=torch.int64).pin_memory()
        self.fid_pin = torch.zeros((B,), dtype=torch.int64).pin_memory()
        self.offs_dev = torch.zeros((B + 1,), dtype=torch.int64, device=device)
        self.fid_dev = torch.zeros((B,), dtype=torch.int64, device=device)
        self.ground = torch.zeros((B, 4), dtype=torch.float64, device=device)
        self.buf = bc.new_buffers(B, max_points=self.cap)
        self.codec_ws = ops.codec_workspace(B, P, bc.M, device)
        # packed device payload + the pinned mirror of every column's buffer (compress_utils.SCHEMA) and of the counts frame_slices cuts them by
        self.qp = torch.empty((self.cap,), dtype=torch.int16, device=device)
        self.sp = torch.empty((B * P,), dtype=torch.int16, device=device)
        self.tot = torch.zeros((2,), dtype=torch.int64, device=device)
        self.qp_pin = torch.empty((self.cap,), dtype=torch.int16).pin_memory()
        self.sp_pin = torch.empty((B * P,), dtype=torch.int16).pin_memory()
        self.bits_pin = torch.empty((B, (P + 7) // 8), dtype=torch.uint8).pin_memory()
        self.model_pin = torch.empty((B, K, 4), dtype=torch.float32).pin_memory()
        self.counts_pin = torch.empty((B, K), dtype=torch.int32).pin_memory()
        self.nnz_pin = torch.empty((B,), dtype=torch.int32).pin_memory()
        self.nseq_pin = torch.empty((B,), dtype=torch.int32).pin_memory()
        self.sal_pin = torch.empty((B, K), dtype=torch.uint8).pin_memory() if bc.general else None
        self.tot_pin = torch.zeros((2,), dtype=torch.int64).pin_memory()
        self.status_pin = torch.zeros((B,), dtype=torch.int32).pin_memory() if bc.dbscan else None   # (rpcc_compress_batch_labels: refused frames)
        # bc.intensity_scale: the intensity payload rows (8 + n bytes of 8 + P each are meaningful), their lengths and orphan counts
        self.int_pin = torch.empty((B, 8 + P), dtype=torch.uint8).pin_memory() if bc.intensity_scale is not None else None
        self.int_n_pin = torch.zeros((2, B), dtype=torch.int32).pin_memory() if bc.intensity_scale is not None else None
        # bc.subpixel_bits: the subpixel payload rows (8 + 2n bytes of 8 + 2P each are meaningful), their lengths and orphan counts
        self.sub_pin = torch.empty((B, 8 + 2 * P), dtype=torch.uint8).pin_memory() if bc.subpixel_bits is not None else None
        self.sub_n_pin = torch.zeros((2, B), dtype=torch.int32).pin_memory() if bc.subpixel_bits is not None else None
        # bc.hidden_points: the hidden_points payload rows (16 + P + 4 rows of the batch's largest frame; made when the first batch is
        # enqueued and whenever the device rows grow), their lengths, orphan and uncarried counts
        self.hid_pin = None
        self.hid_n_pin = torch.zeros((3, B), dtype=torch.int32).pin_memory() if bc.hidden_points else None
        self.hid_rows = 0      # rows of the largest frame staged
        self.h2d_done = torch.cuda.Event()
        self.done = torch.cuda.Event()
        self.n = 0

    def grow(self, cap_points, device):
        """More points than the slot was sized for (dense sweeps, dual returns: a frame may hold more than one point per
        pixel): the point-count-sized buffers are replaced.  Only called while the slot is idle (nothing of it in flight);
        the projection workspace inside BatchBuffers follows by itself (ops.compress_batch)."""
        self.cap = int(cap_points)
        self._point_buffers(device)
        self.qp = torch.empty((self.cap,), dtype=torch.int16, device=device)
        self.qp_pin = torch.empty((self.cap,), dtype=torch.int16).pin_memory()

    def grow_bytes(self, cap_bytes, device):
        """ingest="fields": a chunk of more bytes than the slot was sized for.  Only called while the slot is idle."""
        self.cap_bytes = int(cap_bytes)
        self.chunk_pin = torch.empty((self.cap_bytes,), dtype=torch.uint8).pin_memory()
        self.chunk_dev = torch.empty((self.cap_bytes,), dtype=torch.uint8, device=device)

    def _point_buffers(self, device):
        """The input buffers of cap points: the pinned staging and its device mirror -- floats, or with nclt the records, whose rows
        exist on the device only (no pinned float staging); with fields the files' bytes and a descriptor per frame."""
        if self.fields:
            self.xyz_pin = None
            if not hasattr(self, "chunk_pin"):
                self.grow_bytes(self.cap_bytes, device)
                self.desc_pin = torch.zeros((self.B, pointfile.DESC_WORDS), dtype=torch.int64).pin_memory()
                self.desc_dev = torch.zeros((self.B, pointfile.DESC_WORDS), dtype=torch.int64, device=device)
                self.fstatus_dev = torch.zeros((self.B,), dtype=torch.int32, device=device)
                self.fstatus_pin = torch.zeros((self.B,), dtype=torch.int32).pin_memory()
        elif self.nclt:
            self.xyz_pin = None
            self.rec_pin = torch.empty((self.cap, records.RECORD_BYTES), dtype=torch.uint8).pin_memory()
            self.rec_dev = torch.empty((self.cap, records.RECORD_BYTES), dtype=torch.uint8, device=device)
        else:
            self.xyz_pin = torch.empty((self.cap, self.cols), dtype=torch.float32).pin_memory()
        self.xyz_dev = torch.empty((self.cap, self.cols), dtype=torch.float32, device=device)


class StreamingCompressor:
    """bc: pipeline.BatchCompressor (settings: lidar geometry, cluster count, framework, model, entropy back-end).
    batch: frames per device batch; depth: slots in flight; workers: host threads (staging copies, entropy coding)."""

    def __init__(self, bc, batch=256, depth=4, workers=None, points_per_frame=None, pool=None, ingest="xyz"):
        """ingest: "xyz"  -- frames are [N,>=3] arrays; their first three columns are copied into the pinned slot (12 bytes per
                             point staged and sent over the link; a strided host pass when the arrays are .bin rows);
                   "rows" -- the sweeps AS STORED (dataset/dataset.py:48-50: float32 rows x, y, z, intensity): frames are
                             [N,4] arrays (one contiguous copy each) or .bin PATHS, which are read straight into the pinned
                             slot (file -> pinned buffer -> DMA, no pass over the points on the host); the kernels read
                             the rows with a 16-byte stride (rpcc_batch_io.point_stride_bytes = 16).  16 bytes per point
                             cross the link instead of 12.
                   "nclt" -- NCLT velodyne_sync records (records.py: 8 bytes per point, the intensity byte among them): frames are
                             record-file PATHS, read straight into a pinned record buffer, or uint8 [N,8] arrays; the records cross
                             the link and records.unpack (librpcc_records.so) writes the stored rows on the device, on the compute
                             stream in front of the batch call.  8 bytes per point cross the link; intensity_scale is allowed.
                   "fields" -- .pcd / .ply files (pointfile.py): frames are PATHS.  A worker parses the header, reads the file as it is into
                             the pinned chunk at a 16-byte aligned offset and fills the frame's descriptor; the chunk crosses the link and
                             pointfile.unpack_into (librpcc_fields.so) writes the stored rows on the device, intensity included, in front
                             of the batch call.  A binary_compressed body is LZF-decoded into the chunk by the worker; an ASCII file, or one
                             with a step above RPCC_FIELDS_MAX_STEP, is parsed by the worker into stored rows in the chunk."""
        assert ingest in ("xyz", "rows", "nclt", "fields")
        if bc.intensity_scale is not None and ingest == "xyz":
            raise ValueError('StreamingCompressor: a BatchCompressor with intensity_scale needs ingest="rows" (the fourth column must reach the device); '
                             'ingest="xyz" drops it')
        if bc.subpixel_bits is not None and ingest == "xyz":
            raise ValueError('StreamingCompressor: a BatchCompressor with subpixel_bits needs ingest="rows" (the owner pass reads 16-byte rows); '
                             'ingest="xyz" stages packed points')
        if bc.hidden_points and ingest == "xyz":
            raise ValueError('StreamingCompressor: a BatchCompressor with hidden_points needs ingest="rows" (the owner pass reads 16-byte rows); '
                             'ingest="xyz" stages packed points')
        self.ingest = ingest
        self.bc, self.B, self.depth = bc, int(batch), int(depth)
        self.device = bc.device
        P = bc.T.H * bc.T.W
        # initial capacity of a slot in points (default: one per pixel and frame -- a sweep rarely holds more); a batch with
        # more points makes its slot grow (_Slot.grow), so this is a sizing hint, not a limit
        self.cap = int(points_per_frame if points_per_frame is not None else P) * self.B
        self.grown = 0
        self.pool = pool or ThreadPoolExecutor(workers or min(32, available_cpus()))
        self.copy_stream = torch.cuda.Stream(device=self.device)
        self.compute_stream = torch.cuda.Stream(device=self.device)
        # On this ROCm build a non_blocking copy_ of several hundred MB from pinned memory still holds the calling host thread
        # until the transfer is over (measured: the call returns when the H2D event fires), so the device work of a batch is
        # issued from a thread of its own and the caller stages the next batch meanwhile.
        self.enq_pool = ThreadPoolExecutor(1)
        self.side_stream = torch.cuda.Stream(device=self.device)     # late copies that must not queue behind the next batch
        self.seq_eager = max(1024, self.B * P // 16)                # index-sequence entries fetched with the batch (typical: P/20 per frame)
        self.slots = [_Slot(bc, self.B, self.cap, self.device, cols=3 if ingest == "xyz" else 4, nclt=ingest == "nclt", fields=ingest == "fields") for _ in range(self.depth)]
        self.prof = {"stage": 0.0, "enqueue": 0.0, "collect": 0.0, "drain": 0.0}   # host seconds per phase (diagnostics)
        self.stage_chunks = max(1, min(self.B, 16))      # staging tasks per batch: a few MB each (more, smaller tasks are slower)

    # ---- host staging: frames -> pinned slot (pool threads; numpy releases the GIL inside the copies) -----------------
    def _stage(self, slot, frames, frame_ids):
        n = len(frames)
        assert 0 < n <= self.B
        if self.ingest == "fields":
            return self._stage_fields(slot, frames, frame_ids)
        nclt = self.ingest == "nclt"
        rows = self.ingest == "rows" or nclt      # whole stored elements, files read in place: float rows, or records
        elem = records.RECORD_BYTES if nclt else 16     # bytes of one
        if rows:
            def rows_of(f):
                if not isinstance(f, (str, os.PathLike)):
                    return records.as_records(f).shape[0] if nclt else f.shape[0]
                nbytes = os.path.getsize(f)
                if nbytes % elem:   # the reference's np.fromfile(...).reshape(-1, 4) raises on such a file (dataset/dataset.py:48-50), and so does ingest="xyz"
                    raise ValueError("%s: %d bytes is no whole number of %s" % (f, nbytes, "%d-byte NCLT records" % elem if nclt else
                                                                                 "(x, y, z, intensity) float32 rows"))
                return nbytes // elem
            sizes = np.fromiter((rows_of(f) for f in frames), dtype=np.int64, count=n)
        else:
            sizes = np.fromiter((f.shape[0] for f in frames), dtype=np.int64, count=n)
        offs = np.zeros(self.B + 1, np.int64)
        offs[1:n + 1] = np.cumsum(sizes)
        offs[n + 1:] = offs[n]                       # a short last batch: the missing frames are empty
        if offs[n] > slot.cap:      # the slot is idle here (run() drained it): replace its point-sized buffers, with headroom
            slot.grow(int(offs[n]) + int(offs[n]) // 4, self.device)
            self.grown += 1
        dst = (slot.rec_pin if nclt else slot.xyz_pin).numpy()

        def copy(lo, hi):
            for i in range(lo, hi):
                f = frames[i]
                if not rows:
                    dst[offs[i]:offs[i + 1]] = f[:, :3]   # .bin rows are (x, y, z, intensity): the strided copy drops the 4th column (ingest="rows" keeps it)
                elif isinstance(f, (str, os.PathLike)):       # the file's bytes land in the pinned slot: no pass over the points at all
                    with open(f, "rb", buffering=0) as fh:
                        if os.fstat(fh.fileno()).st_size != elem * int(offs[i + 1] - offs[i]):   # grew or shrank since it was sized
                            raise ValueError("%s changed size while the batch was staged" % f)
                        if offs[i + 1] == offs[i]:
                            continue
                        view = memoryview(dst[offs[i]:offs[i + 1]].reshape(-1).view(np.uint8))
                        got = fh.readinto(view)
                        while 0 < got < len(view):            # (short reads: network file systems)
                            m = fh.readinto(view[got:])
                            if not m:
                                break
                            got += m
                        if got != len(view):
                            raise ValueError("%s changed size while it was read" % f)
                elif nclt:
                    dst[offs[i]:offs[i + 1]] = records.as_records(f)      # (raises for what is no uint8 [N,8] array)
                else:
                    assert f.ndim == 2 and f.shape[1] == 4 and f.dtype == np.float32, 'ingest="rows" takes [N,4] float32 rows or .bin paths'
                    dst[offs[i]:offs[i + 1]] = f           # contiguous rows: one memcpy
            return hi - lo
        step = (n + self.stage_chunks - 1) // self.stage_chunks
        list(self.pool.map(lambda lo: copy(lo, min(lo + step, n)), range(0, n, step)))
        slot.offs_pin.numpy()[:] = offs
        fid = np.zeros(self.B, np.int64)
        fid[:n] = np.asarray(frame_ids if frame_ids is not None else np.arange(n), np.int64)[:n]
        slot.fid_pin.numpy()[:] = fid
        slot.n = n
        slot.hid_rows = int(sizes.max()) if n else 0
        return int(offs[n])

    def _stage_fields(self, slot, frames, frame_ids):
        """ingest="fields": headers first (the chunk's offsets follow from them), then every file into its place in the pinned chunk."""
        n = len(frames)
        for f in frames:
            if not isinstance(f, (str, os.PathLike)):
                raise ValueError('ingest="fields" takes the paths of .pcd / .ply files')
        layouts = list(self.pool.map(pointfile.read_layout, frames))
        direct = [lay.data == "binary" and lay.max_step <= pointfile.MAX_STEP for lay in layouts]
        sizes_f = [os.path.getsize(f) for f in frames]
        # bytes of the chunk a frame takes: the file as it is; else the decompressed body, or the rows a worker makes of it
        need = np.array([sz if d else (lay.body_bytes if lay.data == "binary_compressed" else 16 * lay.n)
                         for lay, d, sz in zip(layouts, direct, sizes_f)], np.int64)
        at = np.zeros(n + 1, np.int64)
        at[1:] = np.cumsum((need + 15) & ~15)          # 16-byte aligned slots
        sizes = np.fromiter((lay.n for lay in layouts), dtype=np.int64, count=n)
        offs = np.zeros(self.B + 1, np.int64)
        offs[1:n + 1] = np.cumsum(sizes)
        offs[n + 1:] = offs[n]
        if offs[n] > slot.cap:
            slot.grow(int(offs[n]) + int(offs[n]) // 4, self.device)
            self.grown += 1
        if at[n] > slot.cap_bytes:
            slot.grow_bytes(int(at[n]) + int(at[n]) // 4, self.device)
            self.grown += 1
        dst = slot.chunk_pin.numpy()
        desc = np.tile(pointfile.stored_layout(0).desc(0), (self.B, 1))      # (the frames a short batch lacks: empty, valid)

        def place(i):
            lay, path, lo = layouts[i], frames[i], int(at[i])
            if direct[i]:
                view = memoryview(dst[lo: lo + sizes_f[i]])
                with open(path, "rb", buffering=0) as fh:
                    got = 0
                    while got < len(view):
                        m = fh.readinto(view[got:])
                        if not m:
                            break
                        got += m
                    if got != len(view) or fh.read(1):
                        raise ValueError("%s changed size while it was read" % path)
                desc[i] = lay.desc(lo + lay.data_off)
            elif lay.data == "binary_compressed":
                with open(path, "rb") as fh:
                    buf = fh.read()
                comp, uncomp = pointfile.compressed_sizes(lay, buf)
                pointfile.lzf_decompress(memoryview(buf)[lay.data_off + 8: lay.data_off + 8 + comp], dst[lo: lo + uncomp], lay.name)
                desc[i] = lay.desc(lo)
            else:       # ASCII, or a step the kernel does not take: the host reader's rows, described as stored rows
                rows = pointfile.read_rows(path)
                if rows.shape[0] != lay.n:
                    raise ValueError("%s changed while it was read" % path)
                dst[lo: lo + 16 * lay.n] = rows.reshape(-1).view(np.uint8)
                desc[i] = pointfile.stored_layout(lay.n).desc(lo)
            return 1
        list(self.pool.map(place, range(n)))
        slot.desc_pin.numpy()[:] = desc
        slot.offs_pin.numpy()[:] = offs
        fid = np.zeros(self.B, np.int64)
        fid[:n] = np.asarray(frame_ids if frame_ids is not None else np.arange(n), np.int64)[:n]
        slot.fid_pin.numpy()[:] = fid
        slot.n, slot.nbytes = n, int(at[n])
        slot.hid_rows = int(sizes.max()) if n else 0
        return int(offs[n])

    # ---- device part: H2D on the copy stream, everything else on the compute stream ------------------------------------
    def _enqueue(self, slot, npts):
        bc = self.bc
        torch.cuda.set_device(self.device)      # (runs on the enqueue thread)
        with torch.cuda.stream(self.copy_stream):
            if slot.fields:
                slot.chunk_dev[:slot.nbytes].copy_(slot.chunk_pin[:slot.nbytes], non_blocking=True)
                slot.desc_dev.copy_(slot.desc_pin, non_blocking=True)
            elif slot.nclt:
                slot.rec_dev[:npts].copy_(slot.rec_pin[:npts], non_blocking=True)
            else:
                slot.xyz_dev[:npts].copy_(slot.xyz_pin[:npts], non_blocking=True)
            slot.offs_dev.copy_(slot.offs_pin, non_blocking=True)
            slot.fid_dev.copy_(slot.fid_pin, non_blocking=True)
            slot.h2d_done.record(self.copy_stream)
        with torch.cuda.stream(self.compute_stream):
            self.compute_stream.wait_event(slot.h2d_done)
            if slot.nclt:     # the records -> the stored rows run_batch reads (16-byte stride), in front of it on this stream
                records.unpack(slot.rec_dev[:npts], out=slot.xyz_dev[:npts])
            if slot.fields:   # the files' bytes -> the stored rows, every frame of the chunk in one launch
                pointfile.unpack_into(slot.chunk_dev[:slot.nbytes], slot.desc_dev, slot.offs_dev, npts, slot.xyz_dev, slot.fstatus_dev)
                slot.fstatus_pin.copy_(slot.fstatus_dev, non_blocking=True)
            # (FPS: one ops.compress_batch; DBSCAN: projection, ground fit, dbscan_segment, ops.compress_batch_labels)
            bc.run_batch(slot.xyz_dev[:npts], slot.offs_dev, slot.ground, slot.buf, frame_ids=slot.fid_dev, max_rows=slot.hid_rows)
            bits, seq, nseq = ops.contour_encode(slot.buf.seg, bc.M, ws=slot.codec_ws)
            ops.pack_payload(slot.buf.q16, slot.buf.nnz, packed=slot.qp, capacity=slot.cap, total=slot.tot[0:1])
            ops.pack_payload(seq.view(torch.int16), nseq, packed=slot.sp, capacity=slot.sp.numel(), total=slot.tot[1:2])
            # D2H of what the container needs (upper bounds: the exact lengths are only known on the device)
            slot.tot_pin.copy_(slot.tot, non_blocking=True)
            slot.nnz_pin.copy_(slot.buf.nnz, non_blocking=True)
            slot.nseq_pin.copy_(nseq, non_blocking=True)
            slot.qp_pin[:npts].copy_(slot.qp[:npts], non_blocking=True)         # sum(nnz) <= points of the batch
            slot.sp_pin[:self.seq_eager].copy_(slot.sp[:self.seq_eager], non_blocking=True)   # usually all of it (see _collect)
            slot.bits_pin.copy_(bits, non_blocking=True)
            slot.model_pin.copy_(slot.buf.model, non_blocking=True)
            slot.counts_pin.copy_(slot.buf.counts, non_blocking=True)
            if slot.status_pin is not None:
                slot.status_pin.copy_(slot.buf.status, non_blocking=True)
            if slot.sal_pin is not None and slot.buf.salience is not None:
                slot.sal_pin.copy_(slot.buf.salience, non_blocking=True)
            if slot.int_pin is not None:      # (run_batch has run ops.intensity_encode on the same rows)
                pay, nb, orphans = slot.buf.intensity
                slot.int_pin.copy_(pay, non_blocking=True)
                slot.int_n_pin[0].copy_(nb, non_blocking=True)
                slot.int_n_pin[1].copy_(orphans, non_blocking=True)
            if slot.sub_pin is not None:      # (run_batch has run ops.subpixel_encode on the same rows)
                pay, nb, orphans = slot.buf.subpixel
                slot.sub_pin.copy_(pay, non_blocking=True)
                slot.sub_n_pin[0].copy_(nb, non_blocking=True)
                slot.sub_n_pin[1].copy_(orphans, non_blocking=True)
            if slot.hid_n_pin is not None:    # (run_batch has run ops.hidden_encode on the same rows)
                pay, nb, orphans, uncarried = slot.buf.hidden
                if slot.hid_pin is None or slot.hid_pin.shape != pay.shape:     # the slot is idle until `done`: nobody reads the old mirror
                    slot.hid_pin = torch.empty(tuple(pay.shape), dtype=torch.uint8).pin_memory()
                slot.hid_pin.copy_(pay, non_blocking=True)
                for k, t in enumerate((nb, orphans, uncarried)):
                    slot.hid_n_pin[k].copy_(t, non_blocking=True)
            slot.keep = (bits, seq, nseq)
            slot.done.record(self.compute_stream)

    # ---- host collection: the batch's payload arrays (views into the pinned buffers) --------------------------------------
    def _collect(self, slot):
        slot.enq.result()                       # the enqueue thread has issued the batch (raises what it raised)
        slot.done.synchronize()
        if slot.fields and slot.fstatus_pin.numpy()[:slot.n].any():      # (the workers validated every header: not expected)
            raise ValueError("librpcc_fields.so refused the layout of frame(s) %s of the batch"
                             % ", ".join(str(i) for i in np.nonzero(slot.fstatus_pin.numpy()[:slot.n])[0]))
        if slot.status_pin is not None:   # a frame DBSCAN gave more labels than max_labels (or a capped union-find): raise as collect() does
            self.bc.check_status(slot.status_pin.numpy()[:slot.n])
        if slot.int_pin is not None:
            self.bc.check_orphans(slot.int_n_pin.numpy()[1, :slot.n])
        if slot.sub_pin is not None:
            self.bc.check_orphans(slot.sub_n_pin.numpy()[1, :slot.n], "subpixel")
        if slot.hid_n_pin is not None:
            self.bc.check_hidden(*(slot.hid_n_pin.numpy()[k, :slot.n] for k in range(3)), slot.hid_pin.numpy()[:slot.n, 12:16])
        stot = int(slot.tot_pin[1])
        if stot > self.seq_eager:
            # an unusually long index sequence: the rest is fetched now, on a stream of its own (the compute stream already
            # holds the next batch, which waits for its H2D copy)
            with torch.cuda.stream(self.side_stream):
                slot.sp_pin[self.seq_eager:stot].copy_(slot.sp[self.seq_eager:stot], non_blocking=True)
            self.side_stream.synchronize()
        # the columns' pinned buffers (compress_utils.SCHEMA), cut per frame by the rule BatchCompressor.collect uses (frame_slices)
        num = lambda t: None if t is None else t.numpy()
        bufs = dict(salience_level=num(slot.sal_pin), contour_map=num(slot.bits_pin), idx_sequence=num(slot.sp_pin), plane_param=num(slot.model_pin),
                    residual_quantized=num(slot.qp_pin), intensity=num(slot.int_pin), subpixel=num(slot.sub_pin),
                    hidden_points=num(slot.hid_pin) if slot.hid_n_pin is not None else None)
        return BatchPayload(self.bc.columns, bufs, num(slot.counts_pin), num(slot.nnz_pin), num(slot.nseq_pin),
                            None if slot.int_pin is None else num(slot.int_n_pin)[0], n=slot.n,
                            nsub=None if slot.sub_pin is None else num(slot.sub_n_pin)[0],
                            nhid=None if slot.hid_n_pin is None else num(slot.hid_n_pin)[0])

    def _encode_chunk(self, payload, lo, hi):
        bc = self.bc
        return pack_frames(bc.bc, [payload.frame(b) for b in range(lo, hi)], uniform=bc.uniform)

    def run(self, batches, sink=None, entropy=True):
        """batches: iterable of (frames, frame_ids) -- frames a list of [N,>=3] float32 arrays (at most `batch` of them),
        frame_ids their identities (or None).  For every batch, in order, sink(index, result) is called with the list of
        .rpcc byte strings (entropy=True) or with the batch's BatchPayload (entropy=False; views into pinned buffers, valid
        inside the sink call only).  The entropy coding of a batch runs on the pool while the next batches are staged and
        computed.  Returns the number of frames processed."""
        submitted = []     # FIFO of (index, slot): on the device, not yet collected
        encoding = []      # FIFO of (index, slot, futures): payloads being entropy-coded from the slot's pinned buffers
        total = 0

        def drain(slot=None):
            # hand finished batches to the sink in order; with `slot` given, until that slot's buffers are free again
            n = 0
            while encoding and (slot is None or any(e[1] is slot for e in encoding)):
                k, _, futs = encoding.pop(0)
                res = [blob for f in futs for blob in f.result()]
                if sink is not None:
                    sink(k, res)
                n += len(res)
            return n

        def finish(item):
            k, slot = item
            payload = self._collect(slot)
            if entropy:   # a few frames per task: the per-frame dictionaries are built on the pool's threads as well
                step = max(1, (payload.n + 4 * self.stage_chunks - 1) // (4 * self.stage_chunks))
                encoding.append((k, slot, [self.pool.submit(self._encode_chunk, payload, lo, min(lo + step, payload.n))
                                           for lo in range(0, payload.n, step)]))
                return 0
            if sink is not None:
                sink(k, payload)
            return payload.n

        for k, (frames, fids) in enumerate(batches):
            slot = self.slots[k % self.depth]
            while any(it[1] is slot for it in submitted):        # (depth 1: the slot's previous batch first)
                total += finish(submitted.pop(0))
            t0 = time.perf_counter()
            total += drain(slot)                                 # its pinned output must not be in use by the entropy coder
            t1 = time.perf_counter()
            npts = self._stage(slot, frames, fids)               # overlaps the device work of the batches in `submitted`
            t2 = time.perf_counter()
            slot.enq = self.enq_pool.submit(self._enqueue, slot, npts)
            t3 = time.perf_counter()
            submitted.append((k, slot))
            while len(submitted) > max(1, self.depth - 2):       # submit(n+1) (and n+2 ...) happened: collect(n)
                total += finish(submitted.pop(0))
            t4 = time.perf_counter()
            self.prof["drain"] += t1 - t0; self.prof["stage"] += t2 - t1; self.prof["enqueue"] += t3 - t2; self.prof["collect"] += t4 - t3
        while submitted:
            total += finish(submitted.pop(0))
        total += drain()
        return total


class _DecodeSlot:
    """What one chunk in flight owns: its stream, the chunk-sized images it is decoded into, and the pinned buffers its results land in."""

    def __init__(self, bd, device):
        n, P = bd.chunk, bd.T.H * bd.T.W + getattr(bd, "hidden_capacity", 0)     # (hidden_points: the hidden points' rows behind the image's)
        self.stream = torch.cuda.Stream(device=device)
        with torch.cuda.device(device):
            self.images = bd.rows_buffers(n)
        self.status_pin = torch.empty((n,), dtype=torch.int32).pin_memory()
        self.offsets_pin = torch.empty((n + 1,), dtype=torch.int64).pin_memory()
        self.nonzero_pin = torch.empty((n,), dtype=torch.int32).pin_memory()
        self.rows_pin = torch.empty((n * P, 4), dtype=torch.float32).pin_memory()     # every point kept: the most a chunk can hold
        self.small_done = torch.cuda.Event()
        self.rows_dev = None
        self.writes = []        # futures of the .bin files being written from rows_pin


class StreamingDecompressor:
    """The decode counterpart of StreamingCompressor.  bd: pipeline.BatchDecompressor (geometry, cluster count, framework, entropy back-end,
    intensity); depth: chunks in flight, each on its own stream with its own pinned buffers; workers: host threads, which read the .rpcc
    files of later chunks and write the .bin files of earlier ones while the device works.  A chunk is bd.chunk frames: its containers go up
    in one copy, are decoded into chunk-sized images that never leave the device, and rows.pack turns those into the files' bytes --
    status, offsets, non-zero counts and rows[:total] are all that comes back.  One process, no children.
    What is decoded follows from bd: a BatchDecompressor(device_trailers=True, hidden_points=True) decodes the hidden points into the
    chunk-sized buffers too and cloud.pack puts their rows behind the image's; hidden_points=True here says the caller expects that."""

    def __init__(self, bd, depth=3, workers=None, pool=None, hidden_points=False):
        if hidden_points and not (getattr(bd, "device_trailers", False) and getattr(bd, "hidden_points", False)):
            raise NotImplementedError("StreamingDecompressor: hidden_points -- the packed rows hold one point per pixel; decode containers with "
                                      "the hidden_points trailer per frame (tools.decompress.decode_frame(..., hidden_points=True)), or hand in a "
                                      "BatchDecompressor(..., hidden_points=True, device_trailers=True)")
        self.bd, self.depth, self.device = bd, max(1, int(depth)), bd.device
        self.pool = pool or ThreadPoolExecutor(workers or min(32, available_cpus()))
        self.slots = [_DecodeSlot(bd, self.device) for _ in range(self.depth)]

    @staticmethod
    def _read(path):
        with open(path, "rb") as f:
            return f.read()

    @staticmethod
    def _write(out_path, rows):
        d = os.path.dirname(out_path)
        if d:
            os.makedirs(d, exist_ok=True)
        rows.tofile(out_path)

    def _enqueue(self, slot, blobs):
        n = len(blobs)
        with torch.cuda.stream(slot.stream):
            status, offsets, rows, nonzero = self.bd.decompress_rows_device(blobs, images=slot.images)
            slot.status_pin[:n].copy_(status, non_blocking=True)
            slot.offsets_pin[:n + 1].copy_(offsets, non_blocking=True)
            slot.nonzero_pin[:n].copy_(nonzero, non_blocking=True)
            slot.small_done.record(slot.stream)
        slot.rows_dev = rows

    def _finish(self, slot, blobs, paths, out_paths, first, on_frame):
        """The chunk's rows to the host and its files to the pool, frame by frame in order; raises at the first frame that is refused."""
        n = len(blobs)
        slot.small_done.synchronize()
        offsets = slot.offsets_pin.numpy()[:n + 1].copy()
        total = int(offsets[n])
        with torch.cuda.stream(slot.stream):
            slot.rows_pin[:total].copy_(slot.rows_dev[:total], non_blocking=True)
        slot.stream.synchronize()
        slot.rows_dev = None
        host = slot.rows_pin.numpy()
        for i, st in enumerate(slot.status_pin.numpy()[:n].tolist()):
            if st == _lib.STREAM_OK:
                rows, nz = host[offsets[i]: offsets[i + 1]], int(slot.nonzero_pin[i])
            else:
                try:
                    if not self.bd.falls_back(st):
                        raise self.bd.refusal(st, first + i)
                    rows, nz = self.bd.rows_fallback(blobs[i], first + i)
                except ValueError as e:
                    raise ValueError("%s: %s" % (paths[i], e)) from e
            slot.writes.append(self.pool.submit(self._write, out_paths[i], rows))
            if on_frame is not None:
                on_frame(first + i, rows.shape[0], nz)

    @staticmethod
    def _settle(slot):
        """The slot's files are on disk (raises what a write raised); its pinned rows are free again."""
        writes, slot.writes = slot.writes, []
        for f in writes:
            f.result()

    def run(self, paths, out_paths, on_frame=None):
        """Decodes the .rpcc files `paths` to the .bin files `out_paths` (directories are made), chunk by chunk with up to `depth` chunks in
        flight.  on_frame(index, rows, nonzero) is called in input order for every frame whose file is on its way.  A frame that cannot be
        decoded raises ValueError naming its path: every frame before it has its complete file, the frame itself and those after it in the
        list have none that this call began.  Returns the number of frames."""
        paths, out_paths = list(paths), list(out_paths)
        assert len(paths) == len(out_paths)
        step = self.bd.chunk
        chunks = [(c0, min(c0 + step, len(paths))) for c0 in range(0, len(paths), step)]
        reads = {}

        def prefetch(k):
            if k < len(chunks) and k not in reads:
                reads[k] = [self.pool.submit(self._read, p) for p in paths[chunks[k][0]: chunks[k][1]]]

        flying = []     # FIFO of (slot, blobs, c0, c1): on the device, not yet finished
        done = 0
        try:
            for k in range(min(self.depth, len(chunks))):
                prefetch(k)
            for k, (c0, c1) in enumerate(chunks):
                slot = self.slots[k % self.depth]
                while any(f[0] is slot for f in flying):      # (depth 1: the slot's previous chunk first)
                    s, blobs, a, b = flying.pop(0)
                    self._finish(s, blobs, paths[a:b], out_paths[a:b], a, on_frame)
                    done = b
                self._settle(slot)
                blobs = [f.result() for f in reads.pop(k)]
                prefetch(k + self.depth)
                self._enqueue(slot, blobs)
                flying.append((slot, blobs, c0, c1))
                while len(flying) >= self.depth and self.depth > 1:
                    s, blobs, a, b = flying.pop(0)
                    self._finish(s, blobs, paths[a:b], out_paths[a:b], a, on_frame)
                    done = b
            while flying:
                s, blobs, a, b = flying.pop(0)
                self._finish(s, blobs, paths[a:b], out_paths[a:b], a, on_frame)
                done = b
        finally:
            # whatever happened: nothing of this call is left running -- streams drained, pending reads dropped, begun files completed
            for s in self.slots:
                s.stream.synchronize()
                s.rows_dev = None
            for futs in reads.values():
                for f in futs:
                    f.cancel()
            err = None
            for s in self.slots:
                try:
                    self._settle(s)
                except Exception as e:      # noqa: BLE001 -- a failed write is reported unless a decode error is already on its way
                    err = err or e
            if err is not None and sys.exc_info()[0] is None:
                raise err
        return done
