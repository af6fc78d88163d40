"""PCTransformer -- mirror of the reference's dataset/transformer.py on the HIP path.

Same constructor, attributes and method names; numpy in, numpy out like the pybind11 op it replaces.
channel_distribute_csv (dataset/transformer.py:13-22,45-48,68-91): the lidar's per-beam elevation table -- row h of the range image is
line h of the CSV, a point goes to the row whose angle is nearest to its elevation, and the last point in input order wins its pixel
(rpcc_project_beams; the specification is tests/beam_table_ref.py).
"""
import csv

import numpy as np
import torch

from . import ops
from .utils import load_yaml


def read_channel_csv(path):
    """dataset/transformer.py:15-22: columns `channel` (read and, as in the reference, never used) and `vertical_angle` in degrees
    -> f64 radians, one per line, in file order."""
    vertical_angle = []
    with open(path, "r") as fin:
        for r in csv.DictReader(fin):
            int(r["channel"])
            vertical_angle.append(float(r["vertical_angle"]))
    return np.radians(np.array(vertical_angle, dtype=np.float64))


class PCTransformer:
    def __init__(self, lidar_cfg=None, channel_distribute_csv=None, device="cuda:0"):
        self.even_dist = channel_distribute_csv is None
        if not self.even_dist:
            self.vertical_angle = read_channel_csv(channel_distribute_csv)
        cfg = load_yaml(lidar_cfg) if isinstance(lidar_cfg, str) else dict(lidar_cfg)
        self.horizontal_FOV = cfg["HORIZONTAL_FOV"] * (np.pi / 180)      # dataset/transformer.py:32-37
        self.vertical_max = cfg["VERTICAL_ANGLE_MAX"] * (np.pi / 180)
        self.vertical_min = cfg["VERTICAL_ANGLE_MIN"] * (np.pi / 180)
        self.vertical_FOV = self.vertical_max - self.vertical_min
        self.H = int(cfg["RANGE_IMAGE_HEIGHT"])
        self.W = int(cfg["RANGE_IMAGE_WIDTH"])
        self.device = torch.device(device)
        if not self.even_dist:   # refused by name: a table of another length (the reference: IndexError, or points in wrong rows), non-finite entries
            try:
                self.vertical_angle = ops.beam_table(self.vertical_angle, self.H)
            except ValueError as e:
                raise ValueError("%s: %s" % (channel_distribute_csv, e)) from None
        self.transform_map = self.create_transform_map()
        self.geom = ops.make_geom(self.H, self.W, self.horizontal_FOV, self.vertical_max, self.vertical_min)
        self._tm_dev = None
        self._beams_dev = None
        self._subpixel_dev = None

    def create_transform_map(self):
        """dataset/transformer.py:41-54."""
        return ops.transform_map(self.H, self.W, self.horizontal_FOV, self.vertical_max, self.vertical_min,
                                 vertical_angle=None if self.even_dist else self.vertical_angle)

    @property
    def beams_dev(self):
        """The table's index on the device (ops.beam_index), uploaded once; None for evenly spaced beams."""
        if self.even_dist:
            return None
        if self._beams_dev is None:
            self._beams_dev = ops.beam_index(self.vertical_angle, self.device)
        return self._beams_dev

    def subpixel_tables(self):
        """The f64 table ops.subpixel_decode reads (ops.subpixel_tables), built once and uploaded once.  Evenly spaced beams only: the
        subpixel channel's rows are the even projection's."""
        if not self.even_dist:
            from .compress_utils import BEAM_TABLE_SUBPIXEL
            raise NotImplementedError(BEAM_TABLE_SUBPIXEL)
        if self._subpixel_dev is None:
            self._subpixel_dev = torch.from_numpy(ops.subpixel_tables(self.H, self.W, self.horizontal_FOV, self.vertical_max,
                                                                      self.vertical_min)).to(self.device)
        return self._subpixel_dev

    @property
    def tm_dev(self):
        if self._tm_dev is None:
            self._tm_dev = torch.from_numpy(self.transform_map).to(self.device)
        return self._tm_dev

    def point_cloud_to_range_image(self, point_cloud):
        """dataset/transformer.py:62-66: [N,3] -> f32 [H,W]."""
        xyz = torch.from_numpy(np.ascontiguousarray(point_cloud[:, :3], dtype=np.float32)).to(self.device)
        offs = torch.tensor([0, xyz.shape[0]], dtype=torch.int64, device=self.device)
        return ops.project(xyz, offs, self.geom, beams=self.beams_dev)[0].cpu().numpy()

    def range_image_to_point_cloud(self, range_image):
        """dataset/transformer.py:94-101: [H,W] or [H,W,1] -> [H,W,3]."""
        if range_image.ndim not in (2, 3):
            assert False
        ri = torch.from_numpy(np.ascontiguousarray(range_image, dtype=np.float32).reshape(1, self.H, self.W)).to(self.device)
        return ops.backproject(ri, self.tm_dev)[0].cpu().numpy()
