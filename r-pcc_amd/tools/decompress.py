#!/usr/bin/env python3
"""Single-frame decompression -- counterpart of the reference's tools/decompress.py on the HIP path.
Nothing about the configuration is stored in the .rpcc file: the decoder needs the same YAML / flags /
lidar type as the encoder (as in the reference).  --eval --original_point_cloud FILE compares the reconstruction with
the original (tools/decompress.py:117-150 of the reference)."""
import os
import sys
import time

BASE_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, BASE_DIR)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rpcc_amd  # noqa: E402,F401
from rpcc_amd import ops  # noqa: E402
from rpcc_amd.compress_utils import (decompress_point_cloud, parse_hidden_payload, parse_intensity_payload, parse_subpixel_payload,  # noqa: E402,F401
                                     read_compressed_bitstream)
from rpcc_amd.dataset import build_dataset  # noqa: E402
from rpcc_amd.tools.compress import make_parser, point_format_of, print_intensity_error, print_quality, resolve_cfg  # noqa: E402


def stream_cluster_num(segment_cfg):
    """cluster_num as decode_frame takes it: the configured value for FPS; None for DBSCAN, whose label count is set by the
    frame, so decode_frame sizes it from the stream's model rows."""
    return None if segment_cfg["segment_method"] == "DBSCAN" else segment_cfg["cluster_num"]


def decode_frame(blob_dict, basic_compressor, transformer, cluster_num, accuracy, level_acc, uniform, want_points=True, decoded=None,
                 intensity=False, subpixel=False, hidden_points=False):
    """decompress_point_cloud + dequantise + predict + back-project (tools/decompress.py:79-112).  cluster_num None
    (DBSCAN, stream_cluster_num): the labels 0 .. rows - 1 of the stream's model rows.  decoded: blob_dict's arrays with the entropy
    stage already undone (basic_compressor.decompress_dicts over a chunk of frames).
    intensity=True: blob_dict holds the container's 'intensity' trailer (unpack_bitstream(..., intensity=True)); a fourth value is
    returned, f32 [H,W], by ops.intensity_decode on the label map just recovered; ValueError when the payload is refused.
    subpixel=True: blob_dict holds the 'subpixel' trailer (unpack_bitstream(..., subpixel=True)); the points come from ops.subpixel_decode
    -- every non-empty pixel's ray turned by its two coded offsets -- instead of ops.backproject; ValueError when the payload is refused.
    hidden_points=True: blob_dict holds the 'hidden_points' trailer (unpack_bitstream(..., hidden_points=True)); the points returned are
    f32 [H*W + m, 3]: the image points in raster order, then the m hidden points in payload order, by ops.hidden_decode (on their pixel's
    centre ray, or turned by their own lateral codes where the payload carries them); ValueError when the payload is refused.  The
    intensity image stays [H,W]: the trailer carries no intensity."""
    H, W = transformer.H, transformer.W
    d = basic_compressor.decompress_dict(blob_dict) if decoded is None else decoded
    # The .rpcc file stores no configuration (as in the reference): a wrong --lidar / cluster_num / framework shows up as
    # payload sizes that do not fit.  Check them here instead of letting the kernels index past their buffers.
    if len(d["plane_param"]) % 16 != 0:
        raise ValueError("plane_param payload is not a whole number of float32 [.,4] rows")
    plane_param = np.frombuffer(d["plane_param"], dtype=np.float32).reshape(-1, 4)
    if cluster_num is None:
        cluster_num = max(plane_param.shape[0] - 2, 1)
    P, K = H * W, cluster_num + 2
    if plane_param.shape[0] > K:
        raise ValueError("bitstream holds %d model rows, the configuration allows cluster_num + 2 = %d" % (plane_param.shape[0], K))
    if len(d["contour_map"]) != (P + 7) // 8:
        raise ValueError("contour_map holds %d bytes, a %dx%d range image needs %d (wrong --lidar?)"
                         % (len(d["contour_map"]), H, W, (P + 7) // 8))
    if len(d["idx_sequence"]) % 2 or len(d["residual_quantized"]) % 2:
        raise ValueError("idx_sequence / residual_quantized payloads are not 16-bit arrays")
    s_chk = np.frombuffer(d["idx_sequence"], dtype=np.uint16)
    n_contour = int(np.unpackbits(np.frombuffer(d["contour_map"], dtype=np.uint8))[:P].sum())
    if s_chk.size != n_contour:
        raise ValueError("idx_sequence holds %d labels, the contour map marks %d runs" % (s_chk.size, n_contour))
    if s_chk.size and int(s_chk.max()) >= plane_param.shape[0]:
        raise ValueError("idx_sequence names label %d but only %d model rows are stored" % (int(s_chk.max()), plane_param.shape[0]))
    if not uniform:
        if "salience_level" not in d:
            raise ValueError("non-uniform framework: the bitstream holds no salience_level payload (written with the uniform framework?)")
        sl_chk = np.frombuffer(d["salience_level"], dtype=np.uint8)
        if sl_chk.size > K:
            raise ValueError("salience_level holds more entries than labels")
        if sl_chk.size < plane_param.shape[0]:
            raise ValueError("salience_level holds %d entries for %d model rows" % (sl_chk.size, plane_param.shape[0]))
        if sl_chk.size and int(sl_chk.max()) >= len(level_acc):
            raise ValueError("salience level %d in the bitstream, the configuration defines %d levels (other level_key_point_num?)"
                             % (int(sl_chk.max()), len(level_acc)))
    dev = transformer.device
    model = torch.zeros((1, K, 4), dtype=torch.float32, device=dev)
    model[0, : plane_param.shape[0]] = torch.from_numpy(plane_param.copy()).to(dev)
    bits = torch.from_numpy(np.frombuffer(d["contour_map"], dtype=np.uint8).copy()[None]).to(dev)
    seq = torch.zeros((1, H * W), dtype=torch.uint16, device=dev)
    s = np.frombuffer(d["idx_sequence"], dtype=np.uint16)
    seq[0, : s.size] = torch.from_numpy(s.copy()).to(dev)
    seg = ops.contour_decode(bits, seq, H, W, cluster_num)
    q = torch.zeros((1, H * W), dtype=torch.int16, device=dev)
    qq = np.frombuffer(d["residual_quantized"], dtype=np.int16)
    n_nonempty = int(((seg.view(torch.int16) if seg.dtype == torch.uint16 else seg) != 1).sum().item())   # (uint16 labels: cluster_num > 254)
    if qq.size != n_nonempty:
        raise ValueError("residual_quantized holds %d values, the label map has %d non-empty pixels" % (qq.size, n_nonempty))
    q[0, : qq.size] = torch.from_numpy(qq.copy()).to(dev)
    if subpixel:
        if "subpixel" not in d:
            raise ValueError("the bitstream holds no subpixel payload (compressed without --subpixel?)")
        parse_subpixel_payload(d["subpixel"], n_nonempty)     # (the refusals in words; the device decoder checks the same)
        tables = transformer.subpixel_tables()
    if hidden_points:
        if "hidden_points" not in d:
            raise ValueError("the bitstream holds no hidden_points payload (compressed without --hidden_points?)")
        hid_bits, _, _, hid_k, _, _ = parse_hidden_payload(d["hidden_points"], n_nonempty)     # (the refusals in words; the device decoder checks the same)
        hid_tables = transformer.subpixel_tables() if hid_bits else None
    centre_rays = want_points and not subpixel
    if uniform:
        rec, pc = ops.decode(seg, q, model, transformer.tm_dev, accuracy, want_points=centre_rays)
    else:
        sal = torch.zeros((1, K), dtype=torch.uint8, device=dev)
        sl = np.frombuffer(d["salience_level"], dtype=np.uint8)
        sal[0, : sl.size] = torch.from_numpy(sl.copy()).to(dev)
        rec, pc = ops.decode(seg, q, model, transformer.tm_dev, list(level_acc), salience=sal, want_points=centre_rays)
    if subpixel and want_points:
        pay = torch.from_numpy(np.frombuffer(d["subpixel"], dtype=np.uint8).copy()[None]).to(dev)
        nbytes = torch.tensor([pay.shape[1]], dtype=torch.int32, device=dev)
        if pay.shape[1] < 8 + 2 * P:      # rpcc_subpixel_decode takes rows of at least 8 + 2P bytes
            pay = torch.cat([pay, torch.zeros((1, 8 + 2 * P - pay.shape[1]), dtype=torch.uint8, device=dev)], 1)
        pc, status = ops.subpixel_decode(pay, nbytes, seg, rec.reshape(1, H, W).contiguous(), tables)
        if int(status[0]) != 0:
            raise ValueError("subpixel payload refused by the device decoder (status %d)" % int(status[0]))
    pts = pc[0].cpu().numpy() if pc is not None else None
    if hidden_points and want_points:
        pay = torch.from_numpy(np.frombuffer(d["hidden_points"], dtype=np.uint8).copy()[None]).to(dev)
        nbytes = torch.tensor([pay.shape[1]], dtype=torch.int32, device=dev)
        hid, count, status = ops.hidden_decode(pay, nbytes, seg, transformer.tm_dev, hid_tables, capacity=hid_k.shape[0])
        if int(status[0]) != 0:
            raise ValueError("hidden_points payload refused by the device decoder (status %d)" % int(status[0]))
        pts = np.concatenate([pts.reshape(-1, 3), hid[0, : int(count[0])].cpu().numpy()])
    out = rec[0].cpu().numpy(), pts, seg[0].cpu().numpy()
    if not intensity:
        return out
    if "intensity" not in d:
        raise ValueError("the bitstream holds no intensity payload (compressed without --intensity?)")
    scale, _ = parse_intensity_payload(d["intensity"], n_nonempty)     # (the refusals in words; the device decoder checks the same)
    pay = torch.from_numpy(np.frombuffer(d["intensity"], dtype=np.uint8).copy()[None]).to(dev)
    nbytes = torch.tensor([pay.shape[1]], dtype=torch.int32, device=dev)
    if pay.shape[1] < 8 + P:      # rpcc_intensity_decode takes rows of at least 8 + P bytes
        pay = torch.cat([pay, torch.zeros((1, 8 + P - pay.shape[1]), dtype=torch.uint8, device=dev)], 1)
    w, status = ops.intensity_decode(pay, nbytes, seg)
    if int(status[0]) != 0:
        raise ValueError("intensity payload refused by the device decoder (status %d)" % int(status[0]))
    return out + (w[0].cpu().numpy(),)


def point_intensity(w, pc):
    """The fourth column of the points decode_frame returned: the intensity image's values, then +0.0 for every hidden point behind them (the
    hidden_points trailer carries no intensity)."""
    w = np.asarray(w, dtype=np.float32).reshape(-1)
    return np.concatenate([w, np.zeros(pc.reshape(-1, 3).shape[0] - w.shape[0], np.float32)])


def decompress(args):
    if args.eval and args.original_point_cloud is None:
        raise ValueError("--eval compares with the original point cloud: set --original_point_cloud")
    cfg, accuracy, segment_cfg, model_cfg, basic_compressor, uniform = resolve_cfg(args)
    # (--input_format: how --original_point_cloud is read; the output is written as float values either way)
    dataset = build_dataset(lidar_type=args.lidar, channel_distribute_csv=getattr(args, "channel_distribute_csv", None),
                            point_format=point_format_of(args))
    level_acc = np.array([accuracy] * len(cfg["level_key_point_num"])) + np.array(cfg["level_delta_acc"])
    t0 = time.time()
    want_w, want_s = getattr(args, "intensity", False), getattr(args, "subpixel", None) is not None
    want_h = getattr(args, "hidden_points", False)
    cd = read_compressed_bitstream(args.input, uniform=uniform, intensity=want_w, subpixel=want_s, hidden_points=want_h)
    rec, pc, seg, *w = decode_frame(cd, basic_compressor, dataset.PCTransformer, stream_cluster_num(segment_cfg), accuracy,
                                    level_acc, uniform, intensity=want_w, subpixel=want_s, hidden_points=want_h)
    t1 = time.time()
    dataset.save_point_cloud_to_file(args.output, pc.reshape(-1, 3), intensity=point_intensity(w[0], pc) if want_w else None)
    print("\nDecompression finished.")
    print("reconstructed point cloud save in ", args.output)
    print("    Decode time: ", t1 - t0)
    print("    Points: ", int((rec != 0).sum()))
    if want_h:
        print("    Hidden points: ", pc.reshape(-1, 3).shape[0] - rec.size)
    if args.eval:
        print("\nStart evaluation...")
        point_cloud, range_image, original = dataset.load_range_image_points_from_file(args.original_point_cloud)
        n_points = int((range_image != 0).sum())
        dif = np.abs(rec - range_image[..., 0])
        bits = os.path.getsize(args.input) * 8
        print("\nCompared with ", args.original_point_cloud)
        print("    BPP: ", bits / n_points)
        print("    Compression Ratio: ", (n_points * 32 * 3) / bits)
        print("    Depth Error (mean): ", float(np.mean(dif)))
        print("    Depth Error (max): ", float(np.max(dif)))
        print_quality(original if want_s or want_h else point_cloud, pc, refined=want_s, hidden=want_h)
        if want_w:
            print_intensity_error(dataset.PCTransformer, dataset.load_rows(args.original_point_cloud), range_image[..., 0], w[0])


if __name__ == "__main__":
    p = make_parser()
    a = p.parse_args()
    print("Input arguments:")
    for key, val in vars(a).items():
        print("{:16} {}".format(key, val))
    decompress(a)
