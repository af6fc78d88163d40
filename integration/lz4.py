"""`import lz4` for the reference's utils/compress_utils.py where the lz4 package is not installed: python-lz4 0.7.0's dumps / loads,
coded on the GPU by rpcc_amd.lz4_codec."""
from rpcc_amd.lz4_codec import dumps, loads  # noqa: F401
