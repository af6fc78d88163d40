"""Data access -- mirror of the reference's dataset/__init__.py:52-69 (build_dataset) and
dataset/dataset.py (DatasetTemplate): .bin / .npy / .txt readers, the lidar registry and the
range-image loader.  use_radius_outlier_removal (dataset/dataset.py:29-35, Open3D's remove_radius_outlier(nb_points=3,
radius=1)) runs on the GPU through outlier.remove_radius_outlier (librpcc_filter.so).  Of the reference's
dataset-specific classes (dataset/datasets/*.py) the one with logic of its own is here: NcltDataset reads NCLT's velodyne_sync
records (nclt_dataset.py:36-63) through records.unpack_host, bit-equal to the reference's preprocessing; the
other three only call Open3D on .pcd files, rewriting each as a .bin with a zero fourth column; here .pcd and .ply files are read as they
are, intensity included, through pointfile.read_rows, and save_point_cloud_to_file writes .pcd as well.  Open3D's
colour output and big-endian .ply stay out of scope."""
import os
import struct

import numpy as np

from . import pointfile, records
from .transformer import PCTransformer

_CFG = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lidar_cfg")

__lidar_cfg__ = {
    "VelodyneVLP16": os.path.join(_CFG, "Velodyne_VLP_16.yaml"),
    "Velodyne32E": os.path.join(_CFG, "Velodyne_HDL_32E.yaml"),
    "Velodyne64E": os.path.join(_CFG, "Velodyne_HDL_64E.yaml"),
    "Velodyne64E_2048": os.path.join(_CFG, "Velodyne_HDL_64E_2048.yaml"),   # BASELINE synthetic geometry
}
__dataset_cfg__ = {
    "KITTI": __lidar_cfg__["Velodyne64E"],
    "KITTI_test": os.path.join(_CFG, "Velodyne_HDL_64E_unofficial.yaml"),
    "NCLT": __lidar_cfg__["Velodyne32E"],
    "Oxford": __lidar_cfg__["Velodyne32E"],
    "HKUSTCampus": __lidar_cfg__["VelodyneVLP16"],
    "NCLT_sync": __lidar_cfg__["Velodyne32E"],      # NCLT as downloaded: velodyne_sync records (point_format "nclt"); "NCLT" reads the preprocessed float .bin
}
__dataset_point_format__ = {"NCLT_sync": "nclt"}


class DatasetTemplate:
    def __init__(self, datalist, dataset_cfg, channel_distribute_csv=None, use_radius_outlier_removal=False,
                 device="cuda:0"):
        self.data_list = []
        if datalist is not None:
            with open(datalist, "r") as f:
                self.data_list = [line.strip() for line in f if line.strip()]
        self.use_radius_outlier_removal = bool(use_radius_outlier_removal)
        self.device = device
        if dataset_cfg is not None:
            self.dataset_cfg = dataset_cfg
            self.PCTransformer = PCTransformer(dataset_cfg, channel_distribute_csv, device=device)
            self.transform_map = self.PCTransformer.transform_map

    def __len__(self):
        return len(self.data_list)

    def __getitem__(self, index):
        """dataset/dataset.py:26-41: with use_radius_outlier_removal the range image and the point cloud come from the filtered points
        (nb_points=3, radius=1); the original point cloud is returned unfiltered."""
        file_name = self.data_list[index]
        original = self.load_data(file_name)
        point_cloud = original
        if self.use_radius_outlier_removal:
            from .outlier import remove_radius_outlier   # raises RpccError without a visible GPU
            point_cloud, _ = remove_radius_outlier(original, nb_points=3, radius=1, device=self.device)
        range_image = np.expand_dims(self.PCTransformer.point_cloud_to_range_image(point_cloud), -1)
        point_cloud = self.PCTransformer.range_image_to_point_cloud(range_image)
        return point_cloud, range_image, original, file_name

    @staticmethod
    def load_data(file):
        """dataset/dataset.py:43-63 -> [N,3]."""
        ext = file.split(".")[-1]
        if ext == "txt":
            pc = np.loadtxt(file)
        elif ext == "bin":
            pc = np.fromfile(file, dtype=np.float32).reshape((-1, 4))
        elif ext in ("npy", "npz"):
            pc = np.load(file)
        elif ext in pointfile.EXTENSIONS:
            pc = pointfile.read_rows(file)
        else:
            assert False, "File type not correct: " + file
        return pc[:, :3]

    @staticmethod
    def load_rows(file):
        """The sweep as stored, with its fourth column (not the reference's: load_data drops it) -> f32 [N,4] rows (x, y, z, intensity),
        from a .bin, or from a .txt / .npy with at least 4 columns.  A .pcd / .ply gives its `intensity` field, or zeros where it has none:
        that is the file's own statement about its points."""
        ext = file.split(".")[-1]
        if ext == "bin":
            return np.fromfile(file, dtype=np.float32).reshape((-1, 4))
        if ext in pointfile.EXTENSIONS:
            return pointfile.read_rows(file)
        if ext == "txt":
            pc = np.loadtxt(file, ndmin=2)
        elif ext == "npy":
            pc = np.load(file)
        else:
            raise ValueError("load_rows: %s -- intensity is read from .bin, .txt or .npy files" % file)
        if pc.ndim != 2 or pc.shape[1] < 4:
            raise ValueError("load_rows: %s holds %s values per point, no intensity column" % (file, pc.shape[1] if pc.ndim == 2 else "?"))
        return np.ascontiguousarray(pc[:, :4], dtype=np.float32)

    def load_range_image_points_from_file(self, file):
        """dataset/dataset.py:65-70."""
        original = self.load_data(file)
        range_image = np.expand_dims(self.PCTransformer.point_cloud_to_range_image(original), -1)
        point_cloud = self.PCTransformer.range_image_to_point_cloud(range_image)
        return point_cloud, range_image, original

    @staticmethod
    def save_point_cloud_to_file(file, point_cloud, color=None, intensity=None):
        """dataset/dataset.py:72-107 (txt / bin / npy / ply / pcd).  intensity (one value per point, not the reference's): the fourth column
        of txt / bin / npy instead of zeros, a fourth float property `intensity` of a ply, a fourth field of a pcd; it goes through the same
        sum != 0 filter.  A pcd is DATA binary, FIELDS x y z [intensity], float32, HEIGHT 1 (pointfile.write_pcd); color is not written."""
        ext = file.split(".")[-1]
        keep = np.where(np.sum(point_cloud, -1) != 0)
        point_cloud = point_cloud[keep]
        if intensity is not None:
            intensity = np.asarray(intensity).reshape(-1)[keep[0]].astype(point_cloud.dtype)
        if ext in ("txt", "bin", "npy", "npz"):
            col4 = np.zeros((point_cloud.shape[0], 1)) if intensity is None else intensity[:, None]
            pc4 = np.concatenate((point_cloud, col4), -1)
            if ext == "txt":
                np.savetxt(file, pc4)
            elif ext == "bin":
                pc4.astype(np.float32).tofile(file)
            else:
                np.save(file, pc4)
        elif ext == "ply":
            with open(file, "wb") as fid:
                fid.write(("ply\nformat binary_little_endian 1.0\nelement vertex %d\nproperty float x\n"
                           "property float y\nproperty float z\n%send_header\n"
                           % (point_cloud.shape[0], "" if intensity is None else "property float intensity\n")).encode())
                body = point_cloud[:, :3] if intensity is None else np.concatenate((point_cloud[:, :3], intensity[:, None]), -1)
                fid.write(np.ascontiguousarray(body, dtype="<f4").tobytes())
        elif ext == "pcd":
            pointfile.write_pcd(file, point_cloud, intensity)
        else:
            assert False, "File type not correct."


class NcltDataset(DatasetTemplate):
    """dataset/datasets/nclt_dataset.py: the files are NCLT velodyne_sync records (8 bytes per point, records.py), not float rows.
    load_data is load_original_utf8_data in the dtype the reference's preprocessing stores (float32); load_rows adds the record's
    intensity byte as the fourth column, where the preprocessing writes 0.  A record file ends in .bin like a float file: the format is
    this class, never guessed from the name or the size."""

    @staticmethod
    def load_data(file):
        return NcltDataset.load_rows(file)[:, :3]

    @staticmethod
    def load_rows(file):
        return records.unpack_host(records.read_records(file))


def build_dataset(datalist=None, dataset_name=None, lidar_type=None, use_radius_outlier_removal=False, device="cuda:0",
                  channel_distribute_csv=None, point_format=None):
    """dataset/__init__.py:52-69.  channel_distribute_csv: the lidar's per-beam elevation table (DatasetTemplate.__init__ of the reference
    passes it to PCTransformer; its registry never sets it).  point_format: None -- float points, by the file's extension --, or "nclt":
    NcltDataset, whose files are velodyne_sync records (the registry name "NCLT_sync" implies it)."""
    records.check_point_format(point_format)
    if dataset_name is not None and point_format is None:
        point_format = __dataset_point_format__.get(dataset_name)
    cls = NcltDataset if point_format == "nclt" else DatasetTemplate
    if dataset_name is not None:
        return cls(datalist, __dataset_cfg__[dataset_name], channel_distribute_csv, use_radius_outlier_removal, device)
    if lidar_type is not None:
        return cls(datalist, __lidar_cfg__[lidar_type], channel_distribute_csv, use_radius_outlier_removal, device)
    return cls(datalist, dataset_cfg=None, use_radius_outlier_removal=use_radius_outlier_removal)
