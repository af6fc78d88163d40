#!/usr/bin/env python3
"""Single-frame compression -- same flags and stage structure as the reference's tools/compress.py,
running on the HIP path.  --eval prints the reference's reconstruction-quality lines: the depth error, then the Chamfer
distance, F-score and point-to-point / point-to-plane PSNR of rpcc_amd.evaluate_metrics (librpcc_eval.so)."""
import argparse
import os
import sys
import time

BASE_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, BASE_DIR)

import numpy as np  # noqa: E402

import rpcc_amd  # noqa: E402,F401
from rpcc_amd.compress_utils import (BasicCompressor, QuantizationModule, compress_point_cloud,  # noqa: E402
                                     decompress_point_cloud, encode_hidden, encode_intensity, encode_subpixel, read_compressed_bitstream,
                                     save_compressed_bitstream)
from rpcc_amd.dataset import build_dataset  # noqa: E402
from rpcc_amd.segment_utils import PointCloudSegment  # noqa: E402
from rpcc_amd.utils import frame_identity, load_compressor_cfg  # noqa: E402

PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class _StreamDecode(argparse.Action):
    """--stream_decode: sets batch_decode as well (the streamed path is the batch decoder with chunks in flight)."""

    def __call__(self, parser, namespace, values, option_string=None):
        namespace.stream_decode = namespace.batch_decode = True


def make_parser(datalist=False):
    p = argparse.ArgumentParser()
    if datalist:
        p.add_argument("--datalist", help="datalist of point cloud files.")
        p.add_argument("--output_dir", help="output folder.")
        p.add_argument("--workers", type=int, default=1, help="host threads for entropy coding and file output (tools/compress_datalist.py:25).")
        p.add_argument("--output", action="store_true", help="print per-frame information.")
        p.add_argument("--batch", type=int, default=64, help="frames per device batch.")
        p.add_argument("--points-per-frame", dest="points_per_frame", type=int, default=None,
                       help="initial staging capacity in points per frame (default H x W; the staging slots grow on demand).")
        p.add_argument("--ingest", choices=("auto", "rows", "xyz"), default="auto",
                       help="rows: .bin sweeps go to the device as stored (x, y, z, intensity rows, 16-byte stride, no host pass); "
                            "xyz: loaded and sliced on the host (12 bytes per point over the link); auto: rows when every file is a .bin.")
        p.add_argument("--gather", action="store_true",
                       help="multi-GPU: every rank entropy-codes its shard, the .rpcc bytes are gathered to rank 0 (RCCL) in "
                            "datalist order and rank 0 writes all files (default: every rank writes its own files).")
        p.add_argument("--gather-round", dest="gather_round", type=int, default=4096, help="--gather: frames per rank and round.")
        p.add_argument("--batch_decode", action="store_true",
                       help="decompress_datalist.py: decode every chunk of files through pipeline.BatchDecompressor (one entropy launch and one "
                            "fused decode call per chunk); the output files are the same.")
        p.add_argument("--stream_decode", action=_StreamDecode, nargs=0, default=False,
                       help="decompress_datalist.py: --batch_decode with several chunks in flight (loader.StreamingDecompressor): the .bin rows are "
                            "packed on the device and only they cross the link, while host threads read later files and write earlier ones; the "
                            "output files are the same.  Implies --batch_decode.")
        p.add_argument("--device_trailers", action="store_true",
                       help="decompress_datalist.py --batch_decode / --stream_decode: decode the --subpixel and --hidden_points trailers on the "
                            "batch path as well (pipeline.BatchDecompressor(device_trailers=True)); without it the two are refused there and "
                            "decoded per frame.  The output files are the same.")
        p.add_argument("--max_labels", type=int, default=None,
                       help="segment_method DBSCAN: the largest label a frame may use in the batch kernels (default and at most 1023; up to 255: "
                            "byte labels on the device).  compress_datalist.py refuses a frame with more; decompress_datalist.py --batch_decode "
                            "decodes such a frame through the per-frame path.")
    else:
        p.add_argument("--input", help="single frame input for static compression.")
        p.add_argument("--output", help="output bitstream.")
        p.add_argument("--original_point_cloud", default=None,
                       help="decompress.py --eval: the original point cloud file to compare the reconstruction with.")
    p.add_argument("--lidar", help="lidar type of this point cloud collection.")
    p.add_argument("--input_format", choices=("float", "nclt"), default="float",
                   help="the point files read: float -- .bin / .txt / .npy of float values, by extension (default); nclt -- NCLT velodyne_sync "
                        "records as downloaded (8 bytes per point: uint16 x, y, z, uint8 intensity, uint8 laser), with no preprocessing step. "
                        "compress tools: the input(s); decompress.py: --original_point_cloud.  A record file also ends in .bin: the format is "
                        "never guessed.")
    p.add_argument("--channel_distribute_csv", default=None, metavar="FILE",
                   help="per-beam elevation table of the lidar (columns channel, vertical_angle in degrees; row h of the range image = line h), "
                        "for beams that are not evenly spaced: e.g. lidar_cfg/Velodyne_HDL_64E_beams.csv with --lidar Velodyne64E.")
    p.add_argument("--compressor_yaml", default=os.path.join(PKG, "cfgs/compressor.yaml"))
    p.add_argument("--basic_compressor", type=str, default=None,
                   help="for manual setting: lz4, bzip2, gzip, deflate, or rans (this build's chunk-parallel GPU format; the reference cannot read it).")
    p.add_argument("--device_entropy", action="store_true",
                   help="basic_compressor deflate / gzip: code the gzip members on the GPU (this build; other bytes, the same decoder).")
    p.add_argument("--device_bzip2", action="store_true",
                   help="basic_compressor bzip2: code the bzip2 streams on the GPU (this build; other bytes, the same decoder).")
    p.add_argument("--rans_delta", action="store_true",
                   help="compress tools, basic_compressor rans: code the residuals through the delta filter (format version 2: a container "
                        "about 0.4 times the size; the decompress tools read both versions and need no flag).")
    p.add_argument("--device_bunzip2", action="store_true",
                   help="decompress tools, basic_compressor bzip2: decode the bzip2 streams on the GPU (this build; bz2.decompress's bytes).")
    p.add_argument("--accuracy", type=float, default=None, help="for manual setting.")
    p.add_argument("--segment_method", type=str, default=None, help="for manual setting.")
    p.add_argument("--cluster_num", type=int, default=None, help="for manual setting.")
    p.add_argument("--DBSCAN_eps", type=float, default=None, help="for manual setting.")
    p.add_argument("--model_method", type=str, default=None, help="for manual setting.")
    p.add_argument("--angle_threshold", type=float, default=None, help="for manual setting.")
    p.add_argument("--nonuniform", action="store_true", help="for manual setting.")
    p.add_argument("--use_radius_outlier_removal", action="store_true",
                   help="remove the points with at most 3 others within 1 m before the projection (the reference's use_radius_outlier_removal, "
                        "Open3D remove_radius_outlier(nb_points=3, radius=1); here on the GPU).")
    p.add_argument("--intensity", action="store_true",
                   help="compress tools: carry the sweep's fourth column (lidar intensity / reflectance) as one byte per non-empty pixel, appended "
                        "to the container where every other reader ignores it; decompress tools: read it and write (x, y, z, intensity).")
    p.add_argument("--intensity_scale", type=float, default=255.0, metavar="S",
                   help="--intensity when compressing: the stored byte is rint(intensity * S) clamped to 0 .. 255 (default 255; 100 returns a "
                        "KITTI sweep's values bit for bit).  The scale is stored in the container: decompressing takes no scale.")
    p.add_argument("--subpixel", type=int, nargs="?", default=None, const=SUBPIXEL_FLAG, metavar="BITS",
                   help="compress tools: --subpixel BITS (1 .. 4) carries where inside its pixel's cell every kept point lies, BITS bits per "
                        "axis, one more array appended to the container where every other reader ignores it; decompress tools: --subpixel "
                        "(the bits are stored in the container) reads it and turns every decoded point off its pixel's centre ray by the "
                        "coded offsets.  --eval then compares the refined points with the original points, not with the pixel centres.")
    p.add_argument("--hidden_points", action="store_true",
                   help="compress tools: carry the points that share a pixel with the one the range image keeps (a quarter of a 64-beam sweep), "
                        "a count per non-empty pixel and a 16-bit range code per point, one more array appended last to the container where "
                        "every other reader ignores it; with --subpixel BITS every such point also carries lateral codes of that width.  "
                        "decompress tools: read it and write these points behind the image points.  The trailer carries no intensity: with "
                        "--intensity the fourth column of such a row is 0.  --eval then compares the original points with the image points "
                        "plus the hidden points.")
    p.add_argument("--eval", action="store_true", help="evaluate the reconstruction quality.")
    p.add_argument("--cpu", action="store_true", help="accepted for compatibility; the HIP path has no CPU mode.")
    p.add_argument("--seed", type=int, default=0, help="seed of the ground / plane RANSAC (this build).")
    p.add_argument("--fps_fma", type=int, default=None, choices=(0, 1, 2),
                   help="FPS distance as the reference's CUDA binary may contract it (0 un-fused = default, 1 fma(dz,dz,fma(dx,dx,dy*dy)), "
                        "2 fma(dz,dz,fma(dy,dy,dx*dx))); sets RPCC_FPS_FMA.")
    p.add_argument("--fps_tie_cuda", action="store_true",
                   help="FPS ties between exactly equal distances resolved like the CUDA kernel's reduction tree (default: lowest "
                        "index); sets RPCC_FPS_TIE_CUDA.")
    return p


SUBPIXEL_FLAG = -1      # --subpixel without BITS (the decompress tools' form)


def subpixel_bits_of(args):
    """--subpixel BITS of the compress tools: None (off) or 1 .. 4; ValueError for the flag without BITS or with another value."""
    bits = getattr(args, "subpixel", None)
    if bits is None:
        return None
    if bits == SUBPIXEL_FLAG:
        raise ValueError("--subpixel BITS: compressing needs the number of bits per axis, 1 .. 4")
    from rpcc_amd import ops
    return ops.check_subpixel_bits(bits)


def point_format_of(args):
    """--input_format as build_dataset / BatchCompressor / StreamingCompressor name it: None (float points) or "nclt"."""
    return "nclt" if getattr(args, "input_format", "float") == "nclt" else None


def apply_fps_mode(args):
    """--fps_fma / --fps_tie_cuda -> the environment variables every FPS call of this build reads (ops.compress_batch,
    segment_utils.PointCloudSegment.segment)."""
    if getattr(args, "fps_fma", None) is not None:
        os.environ["RPCC_FPS_FMA"] = str(args.fps_fma)
    if getattr(args, "fps_tie_cuda", False):
        os.environ["RPCC_FPS_TIE_CUDA"] = "1"


def resolve_cfg(args):
    """tools/compress.py:45-84: YAML values overridden by the individual flags."""
    cfg = load_compressor_cfg(args.compressor_yaml)
    accuracy = cfg["accuracy"] * 2
    segment_cfg = {"segment_method": cfg["segment_method"], "ground_vertical_threshold": cfg["ground_threshold"],
                   "cluster_num": cfg["cluster_num"], "DBSCAN_eps": cfg["DBSCAN_eps"]}
    model_cfg = {"model_method": cfg["modeling_method"], "angle_threshold": cfg["plane_angle_threshold"]}
    bc = BasicCompressor(compressor_yaml=args.compressor_yaml, device_entropy=getattr(args, "device_entropy", False),
                         device_bunzip2=getattr(args, "device_bunzip2", False), device_bzip2=getattr(args, "device_bzip2", False),
                         rans_delta=getattr(args, "rans_delta", False))
    if args.basic_compressor is not None:
        bc.set_method(args.basic_compressor)
    if args.accuracy is not None:
        accuracy = args.accuracy * 2
    for key, dst, name in (("segment_method", segment_cfg, "segment_method"), ("cluster_num", segment_cfg, "cluster_num"),
                           ("DBSCAN_eps", segment_cfg, "DBSCAN_eps"), ("model_method", model_cfg, "model_method"),
                           ("angle_threshold", model_cfg, "angle_threshold")):
        if getattr(args, key) is not None:
            dst[name] = getattr(args, key)
    uniform = False if args.nonuniform else cfg["compress_framework"] == "uniform"
    return cfg, accuracy, segment_cfg, model_cfg, bc, uniform


def make_quantizer(cfg, accuracy, uniform):
    if uniform:
        return QuantizationModule(accuracy)
    return QuantizationModule(accuracy, uniform=False, level_kp_num=tuple(cfg["level_key_point_num"]),
                              level_dacc=tuple(cfg["level_delta_acc"]), ground_salience_level=cfg["ground_salience_level"],
                              feature_region=cfg["feature_region"], segments=cfg["segments"], sharp_num=cfg["sharp_num"],
                              less_sharp_num=cfg["less_sharp_num"], flat_num=cfg["flat_num"])


def print_hidden_counts(carried, uncarried):
    """--hidden_points: what the trailer carries, and what it does not when that is not nothing."""
    print("    Hidden points carried: ", int(carried))
    if int(uncarried):
        print("    Hidden points not carried (empty pixel, range code past 65535, more than 255 in a pixel): ", int(uncarried))


def print_quality(point_cloud, point_cloud_rec, refined=False, hidden=False):
    """The four metric lines of the reference's --eval (tools/compress.py:185-192, tools/decompress.py:146-150).  refined (--subpixel):
    point_cloud is the original point list, not the back-projected range image, and a line says so.  hidden (--hidden_points):
    point_cloud is the original point list and point_cloud_rec the image points followed by the hidden points, and a line says so."""
    from rpcc_amd.evaluate_metrics import calc_chamfer_distance, calc_point_to_point_plane_psnr
    chamfer = calc_chamfer_distance(point_cloud, point_cloud_rec, out=False)
    point_to_point, point_to_plane = calc_point_to_point_plane_psnr(point_cloud, point_cloud_rec, out=False)
    if refined:
        print("    (subpixel: the refined points against the original points)")
    if hidden:
        print("    (hidden_points: the image points and the hidden points against the original points)")
    print("    Chamfer Distance (mean): ", chamfer["mean"])
    print("    F1 score (threshold=0.02): ", chamfer["f_score"])
    print("    Point-to-Point PSNR (r=59.7): ", point_to_point["psnr_mean"])
    print("    Point-to-Plane PSNR (r=59.7): ", point_to_plane["psnr_mean"])


def load_intensity_rows(dataset, path, filtered):
    """--intensity: the frame's rows (x, y, z, intensity), after the radius filter when it is on (the rows its index keeps)."""
    rows = dataset.load_rows(path)
    if filtered:
        from rpcc_amd.outlier import remove_radius_outlier
        rows = rows[remove_radius_outlier(rows, nb_points=3, radius=1)[1]]
    return rows


def print_intensity_error(transformer, rows, range_image, w_rec):
    """--eval --intensity: the decoded intensities against the owners' intensities of the original, over the non-empty pixels."""
    import torch
    from rpcc_amd import ops
    dev = transformer.device
    rows_d = torch.from_numpy(np.ascontiguousarray(rows[:, :4], dtype=np.float32)).to(dev)
    ri = torch.from_numpy(np.ascontiguousarray(range_image, dtype=np.float32).reshape(1, transformer.H, transformer.W)).to(dev)
    own = torch.empty_like(ri)
    offs = torch.tensor([0, rows_d.shape[0]], dtype=torch.int64, device=dev)
    ops.intensity_encode(rows_d, offs, transformer.geom, ri, 1.0, owner_intensity=own)
    set_ = (ri != 0)[0].cpu().numpy()
    dif = np.abs(np.asarray(w_rec, dtype=np.float64).reshape(set_.shape) - own[0].cpu().numpy())[set_]
    print("    Intensity Error (max): ", float(dif.max()) if dif.size else 0.0)
    print("    Intensity Error (mean): ", float(dif.mean()) if dif.size else 0.0)


def compress_wide(args, cfg, accuracy, segment_cfg, model_cfg, basic_compressor, uniform):
    """cluster_num above 254 (labels as uint16): the per-stage mirror classes keep labels in a byte, so the frame goes through the batch front-end
    (pipeline.BatchCompressor -> rpcc_compress_batch_wide) as a batch of one.  Same container, same decoder."""
    from rpcc_amd.pipeline import BatchCompressor
    dataset = build_dataset(lidar_type=args.lidar, channel_distribute_csv=getattr(args, "channel_distribute_csv", None),
                            point_format=point_format_of(args))
    t0 = time.time()
    want_w, sub_bits, want_h = getattr(args, "intensity", False), subpixel_bits_of(args), getattr(args, "hidden_points", False)
    if want_w:     # the rows as stored (filtered like the points): the batch front-end makes the payload from its own range image
        frame = load_intensity_rows(dataset, args.input, getattr(args, "use_radius_outlier_removal", False))
    else:
        frame = dataset.load_data(args.input)
        if getattr(args, "use_radius_outlier_removal", False):
            from rpcc_amd.outlier import remove_radius_outlier
            frame, _ = remove_radius_outlier(frame, nb_points=3, radius=1)
    bc = BatchCompressor(dataset.PCTransformer, cluster_num=segment_cfg["cluster_num"], accuracy=accuracy / 2,
                         ground_threshold=segment_cfg["ground_vertical_threshold"], uniform=uniform, model_method=model_cfg["model_method"],
                         compressor_cfg=dict(cfg), basic_compressor=basic_compressor.method_name, seed=args.seed,
                         device_entropy=basic_compressor.device_entropy, device_bzip2=basic_compressor.device_bzip2,
                         rans_delta=basic_compressor.rans_delta, intensity_scale=args.intensity_scale if want_w else None,
                         subpixel_bits=sub_bits, hidden_points=want_h)
    blob = bc.compress([frame], frame_ids=[frame_identity(args.input)])[0]
    with open(args.output, "wb") as f:
        f.write(blob)
    t1 = time.time()
    buf = bc._buf
    point_num = int((buf.ri[0] != 0).sum().item())
    print("\nCompression finished (cluster_num = %d: uint16 labels, batch front-end)." % segment_cfg["cluster_num"])
    print("binary bitstream save in ", args.output)
    print("    Total time cost: ", t1 - t0)
    bits = os.path.getsize(args.output) * 8
    print("\nCompression Results: ")
    print("    Compression ratio: ", (point_num * 32 * 3) / bits)
    print("    BPP: ", bits / point_num)
    if want_h:
        print_hidden_counts(bc.hidden_carried[0], bc.hidden_uncarried[0])
    if args.eval:
        from rpcc_amd.tools.decompress import decode_frame
        level_acc = np.array([accuracy] * len(cfg["level_key_point_num"])) + np.array(cfg["level_delta_acc"])
        want_s = sub_bits is not None
        rec, pc_s, _, *w = decode_frame(read_compressed_bitstream(args.output, uniform=uniform, intensity=want_w, subpixel=want_s, hidden_points=want_h),
                                        basic_compressor, dataset.PCTransformer, segment_cfg["cluster_num"], accuracy, level_acc, uniform,
                                        want_points=want_s or want_h, intensity=want_w, subpixel=want_s, hidden_points=want_h)
        ri = buf.ri[0].cpu().numpy()
        dif = np.abs(rec - ri)   # every pixel, empty ones included, as compress() below and tools/compress.py:172-181
        bound = accuracy + (0.0 if uniform else 0.06) + 0.00001
        print("\nReconstruction quality: ")
        print("    Depth Error (mean): ", float(np.mean(dif)))
        print("    Depth Error (max): ", float(np.max(dif)))
        if float(np.max(dif)) > bound:
            raise AssertionError("Reconstruction error... Please check...")
        T = dataset.PCTransformer
        if want_s or want_h:
            print_quality(frame[:, :3], pc_s, refined=want_s, hidden=want_h)
        else:
            print_quality(T.range_image_to_point_cloud(ri), T.range_image_to_point_cloud(rec))
        if want_w:
            print_intensity_error(T, frame, ri, w[0])


def compress(args):
    apply_fps_mode(args)
    cfg, accuracy, segment_cfg, model_cfg, basic_compressor, uniform = resolve_cfg(args)
    from rpcc_amd import ops
    # DBSCAN: always the per-frame stages here (compress_datalist.py batches it: pipeline.BatchCompressor(segment_method="DBSCAN")); cluster_num does not apply
    if segment_cfg["segment_method"] != "DBSCAN" and ops.is_wide(ops.check_cluster_num(segment_cfg["cluster_num"])):
        return compress_wide(args, cfg, accuracy, segment_cfg, model_cfg, basic_compressor, uniform)
    filtered = getattr(args, "use_radius_outlier_removal", False)
    dataset = build_dataset(lidar_type=args.lidar, use_radius_outlier_removal=filtered,
                            channel_distribute_csv=getattr(args, "channel_distribute_csv", None), point_format=point_format_of(args))
    model_num = segment_cfg["cluster_num"] + 1
    pc_seg = PointCloudSegment(dataset.transform_map, seed=args.seed, frame_id=frame_identity(args.input))

    t_init = time.time()
    if filtered:     # filtered per frame through the dataset (dataset/dataset.py:26-41)
        dataset.data_list = [args.input]
        point_cloud, range_image, original_point_cloud, _ = dataset[0]
    else:
        point_cloud, range_image, original_point_cloud = dataset.load_range_image_points_from_file(args.input)
    point_num = int((point_cloud[..., 0] != 0).sum())
    t_load_data = time.time()
    seg_idx, ground_model = pc_seg.segment(point_cloud, range_image, segment_cfg, cpu=args.cpu)
    t_segmentation = time.time()
    cluster_models = pc_seg.cluster_modeling(point_cloud, range_image, seg_idx, model_cfg)
    model_param = np.concatenate((ground_model.reshape(1, 4), cluster_models), 0)
    t_modeling = time.time()
    range_image_pred = pc_seg.intra_predict(seg_idx, model_param)
    residual = range_image - range_image_pred
    t_intra_pred = time.time()
    QM = make_quantizer(cfg, accuracy, uniform)
    residual_quantized, salience_level, key_point_map = QM.quantize_residual(residual, seg_idx, point_cloud, range_image)
    t_quantization = time.time()
    want_w, rows, payload = getattr(args, "intensity", False), None, None
    if want_w:     # the frame's rows against the range image they were projected to
        rows = load_intensity_rows(dataset, args.input, filtered)
        payload, _ = encode_intensity(dataset.PCTransformer, rows, range_image[..., 0], args.intensity_scale)
    sub_bits, sub_payload, kept = subpixel_bits_of(args), None, None
    if sub_bits is not None:     # the points the range image was made of (after the radius filter when it is on)
        kept = rows if rows is not None else original_point_cloud
        if filtered and rows is None:
            from rpcc_amd.outlier import remove_radius_outlier
            kept, _ = remove_radius_outlier(original_point_cloud, nb_points=3, radius=1)
        sub_payload, _ = encode_subpixel(dataset.PCTransformer, kept, range_image[..., 0], sub_bits)
    want_h, hid_payload, hid_uncarried = getattr(args, "hidden_points", False), None, 0
    if want_h:     # the same points; lateral codes of --subpixel's width where that is given
        if kept is None:
            kept = rows if rows is not None else original_point_cloud
            if filtered and rows is None:
                from rpcc_amd.outlier import remove_radius_outlier
                kept, _ = remove_radius_outlier(original_point_cloud, nb_points=3, radius=1)
        hid_payload, hid_uncarried = encode_hidden(dataset.PCTransformer, kept, range_image[..., 0], accuracy, sub_bits or 0)
    original_data, compressed_data = compress_point_cloud(basic_compressor, model_param, seg_idx, salience_level,
                                                          residual_quantized, full=False, intensity=payload, subpixel=sub_payload,
                                                          hidden_points=hid_payload)
    t_basic_compressor = time.time()
    save_compressed_bitstream(args.output, compressed_data, uniform=uniform)
    t_save = time.time()

    print("\nCompression finished.")
    print("binary bitstream save in ", args.output)
    print("\nTime Cost:")
    print("    Load data: ", t_load_data - t_init)
    print("    Segmentation module: ", t_segmentation - t_load_data)
    print("    Modeling module: ", t_modeling - t_segmentation)
    print("    Intra-prediction module: ", t_intra_pred - t_modeling)
    print("    Quantization module: ", t_quantization - t_intra_pred)
    print("    Basic compressor module (", basic_compressor.method_name, "): ", t_basic_compressor - t_quantization)
    print("    Save binary file: ", t_save - t_basic_compressor)
    print("    Total time cost: ", t_save - t_init)
    print("    Total time cost without loading data: ", t_save - t_load_data)
    bits = os.path.getsize(args.output) * 8
    print("\nCompression Results: ")
    print("    Compression ratio: ", (point_num * 32 * 3) / bits)
    print("    BPP: ", bits / point_num)
    if want_h:
        print_hidden_counts(int(np.frombuffer(hid_payload[12:16].tobytes(), "<u4")[0]), hid_uncarried)
    print("\n")

    if args.eval:
        cd = read_compressed_bitstream(args.output, uniform=uniform)
        rq, seg2, sal2, plane_param = decompress_point_cloud(cd, basic_compressor, model_param.shape[0],
                                                             dataset.transform_map.shape[0], dataset.transform_map.shape[1])
        QM2 = make_quantizer(cfg, accuracy, uniform)
        res2 = QM2.dequantize_residual(rq, seg2, sal2)
        rec = pc_seg.intra_predict(seg2, plane_param) + res2
        dif = np.abs(rec - range_image)
        bound = accuracy + (0.0 if uniform else 0.06) + 0.00001
        print("\nReconstruction quality: ")
        print("    Depth Error (mean): ", float(np.mean(dif)))
        print("    Depth Error (max): ", float(np.max(dif)))
        if float(np.max(dif)) > bound:
            raise AssertionError("Reconstruction error... Please check...")
        want_s = sub_bits is not None
        if want_s or want_h:
            from rpcc_amd.tools.decompress import decode_frame
            level_acc = np.array([accuracy] * len(cfg["level_key_point_num"])) + np.array(cfg["level_delta_acc"])
            refined = decode_frame(read_compressed_bitstream(args.output, uniform=uniform, intensity=want_w, subpixel=want_s, hidden_points=want_h),
                                   basic_compressor, dataset.PCTransformer,
                                   None if segment_cfg["segment_method"] == "DBSCAN" else segment_cfg["cluster_num"],
                                   accuracy, level_acc, uniform, subpixel=want_s, hidden_points=want_h)[1]
            print_quality(np.asarray(kept)[:, :3], refined, refined=want_s, hidden=want_h)
        else:
            print_quality(point_cloud, dataset.PCTransformer.range_image_to_point_cloud(rec))
        if want_w:
            from rpcc_amd.tools.decompress import decode_frame
            level_acc = np.array([accuracy] * len(cfg["level_key_point_num"])) + np.array(cfg["level_delta_acc"])
            w = decode_frame(read_compressed_bitstream(args.output, uniform=uniform, intensity=True, subpixel=sub_bits is not None, hidden_points=want_h),
                             basic_compressor, dataset.PCTransformer,
                             None if segment_cfg["segment_method"] == "DBSCAN" else segment_cfg["cluster_num"], accuracy, level_acc, uniform,
                             want_points=False, intensity=True)[3]
            print_intensity_error(dataset.PCTransformer, rows, range_image[..., 0], w)


if __name__ == "__main__":
    a = make_parser().parse_args()
    print("Input arguments:")
    for key, val in vars(a).items():
        print("{:16} {}".format(key, val))
    compress(a)
