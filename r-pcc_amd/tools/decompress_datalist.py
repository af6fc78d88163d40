#!/usr/bin/env python3
"""Datalist decompression -- counterpart of the reference's tools/decompress_datalist.py: every
`.rpcc` named in the datalist is decoded and written as <output_dir>/<path>.bin."""
import os
import sys
from concurrent import futures

BASE_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, BASE_DIR)

import numpy as np  # noqa: E402

import rpcc_amd  # noqa: E402,F401
from rpcc_amd.compress_utils import read_compressed_bitstream  # noqa: E402
from rpcc_amd.dataset import build_dataset  # noqa: E402
from rpcc_amd.sharding import shard_indices  # noqa: E402
from rpcc_amd.tools.compress import make_parser, point_format_of, resolve_cfg  # noqa: E402
from rpcc_amd.tools.decompress import decode_frame, point_intensity, stream_cluster_num  # noqa: E402


CHUNK = 32   # .rpcc files read and entropy-decoded together


def output_path(args, name):
    rel = name[1:] if name.startswith("/") else name
    out = os.path.join(args.output_dir, rel)
    return out.replace(out.split(".")[-1], "bin")


def decompress_batched(args, dataset, mine, cluster_num, accuracy, level_acc, uniform, basic_compressor):
    """--batch_decode: the chunks through pipeline.BatchDecompressor (the files' bytes as they are, one device pass per chunk)."""
    from rpcc_amd.pipeline import BatchDecompressor
    # (DBSCAN streams: cluster_num None -- the label count is the frame's; the batch decodes them under a label cap)
    cap = (getattr(args, "max_labels", None) or 1023) if cluster_num is None else None
    # (--device_trailers: the subpixel and hidden_points trailers on this path too; without it decompress() has refused them by now)
    trailers = dict(subpixel=getattr(args, "subpixel", None) is not None, hidden_points=getattr(args, "hidden_points", False),
                    device_trailers=True) if getattr(args, "device_trailers", False) else {}
    bd = BatchDecompressor(dataset.PCTransformer, cluster_num, accuracy, uniform=uniform, level_acc=level_acc, basic_compressor=basic_compressor,
                           max_labels=cap, intensity=getattr(args, "intensity", False), **trailers)
    if getattr(args, "stream_decode", False):
        return decompress_streamed(args, bd, [dataset.data_list[i] for i in mine])
    for c0 in range(0, len(mine), CHUNK):
        names = [dataset.data_list[i] for i in mine[c0: c0 + CHUNK]]
        blobs = []
        for name in names:
            with open(name, "rb") as f:
                blobs.append(f.read())
        for name, (rec, pc, _, *w) in zip(names, bd.decompress(blobs)):
            out = output_path(args, name)
            os.makedirs(os.path.dirname(out), exist_ok=True)
            dataset.save_point_cloud_to_file(out, pc.reshape(-1, 3), intensity=(point_intensity(w[0], pc) if bd.hidden_points else w[0].reshape(-1)) if w else None)
            if args.output:
                print("%s -> %s (%d points)" % (name, out, int((rec != 0).sum())))


def decompress_streamed(args, bd, names):
    """--stream_decode: this rank's shard through loader.StreamingDecompressor -- the .bin rows are made on the device, several chunks are
    in flight, and the pool's threads (--workers; left at 1, the loader's own default) read and write files meanwhile.  The same files as
    --batch_decode."""
    from rpcc_amd.loader import StreamingDecompressor
    outs = [output_path(args, name) for name in names]
    report = (lambda i, rows, nonzero: print("%s -> %s (%d points)" % (names[i], outs[i], nonzero))) if args.output else None
    workers = int(getattr(args, "workers", 1) or 1)
    StreamingDecompressor(bd, workers=workers if workers > 1 else None, hidden_points=bd.hidden_points).run(names, outs, on_frame=report)


def decompress(args):
    rank =int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    device = "cuda:%d" % int(os.environ.get("LOCAL_RANK", "0"))
    refused = getattr(args, "batch_decode", False) and not getattr(args, "device_trailers", False)
    if refused and getattr(args, "subpixel", None) is not None:     # (before anything is read or built)
        raise NotImplementedError("--%s with --subpixel: the batch decoder back-projects along the pixels' centre rays; decode containers with "
                                  "the subpixel trailer without --batch_decode / --stream_decode (the per-frame path), or add --device_trailers"
                                  % ("stream_decode" if getattr(args, "stream_decode", False) else "batch_decode"))
    if refused and getattr(args, "hidden_points", False):
        raise NotImplementedError("--%s with --hidden_points: the batch decoder returns one point per pixel; decode containers with the "
                                  "hidden_points trailer without --batch_decode / --stream_decode (the per-frame path), or add --device_trailers"
                                  % ("stream_decode" if getattr(args, "stream_decode", False) else "batch_decode"))
    cfg, accuracy, segment_cfg, model_cfg, basic_compressor, uniform = resolve_cfg(args)
    # (--input_format: how the dataset reads original point files; this tool reads none, its outputs are float .bin files either way)
    dataset = build_dataset(datalist=args.datalist, lidar_type=args.lidar, device=device,
                            channel_distribute_csv=getattr(args, "channel_distribute_csv", None), point_format=point_format_of(args))
    level_acc = np.array([accuracy] * len(cfg["level_key_point_num"])) + np.array(cfg["level_delta_acc"])
    mine = list(shard_indices(len(dataset), rank, world))
    if getattr(args, "batch_decode", False):
        return decompress_batched(args, dataset, mine, stream_cluster_num(segment_cfg), accuracy, level_acc, uniform, basic_compressor)
    for c0 in range(0, len(mine), CHUNK):
        names = [dataset.data_list[i] for i in mine[c0: c0 + CHUNK]]
        want_w, want_s = getattr(args, "intensity", False), getattr(args, "subpixel", None) is not None
        want_h = getattr(args, "hidden_points", False)
        cds = [read_compressed_bitstream(name, uniform=uniform, intensity=want_w, subpixel=want_s, hidden_points=want_h) for name in names]
        for name, cd, d in zip(names, cds, basic_compressor.decompress_dicts(cds)):   # the chunk's entropy stage in one call where the back-end has one
            rec, pc, _, *w = decode_frame(cd, basic_compressor, dataset.PCTransformer, stream_cluster_num(segment_cfg), accuracy,
                                          level_acc, uniform, decoded=d, intensity=want_w, subpixel=want_s, hidden_points=want_h)
            rel = name[1:] if name.startswith("/") else name
            out = os.path.join(args.output_dir, rel)
            out = out.replace(out.split(".")[-1], "bin")
            os.makedirs(os.path.dirname(out), exist_ok=True)
            dataset.save_point_cloud_to_file(out, pc.reshape(-1, 3), intensity=point_intensity(w[0], pc) if w else None)
            if args.output:
                print("%s -> %s (%d points)" % (name, out, int((rec != 0).sum())))


if __name__ == "__main__":
    a = make_parser(datalist=True).parse_args()
    decompress(a)
