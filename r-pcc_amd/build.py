"""Builds librpcc_hip.so (the C-ABI HIP library) in-tree with hipcc for gfx950."""
import os
import subprocess

_HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(_HERE, "csrc", "rpcc_hip.hip")
DEPS = [os.path.join(_HERE, "csrc", f) for f in sorted(os.listdir(os.path.join(_HERE, "csrc")))] + \
       [os.path.join(os.path.dirname(_HERE), "include", "rpcc_hip.h")]
LIB = os.path.join(_HERE, "lib", "librpcc_hip.so")
HOST_SRC = os.path.join(_HERE, "csrc", "rpcc_host.c")
HOST_LIB = os.path.join(_HERE, "lib", "librpcc_host.so")
# the host LZF decoder of .pcd binary_compressed bodies: a source of its own (csrc_fields/), outside DEPS and source_digest()
HOST_LZF_SRC = os.path.join(_HERE, "csrc_fields", "rpcc_lzf.c")
HOST_LZF_DEPS = [HOST_LZF_SRC, os.path.join(_HERE, "csrc_fields", "lzf_decode.h")]


def _side_library(subdir, src, header, lib, shared=("csrc_tile",)):
    """(src, deps, lib) of a HIP library of its own beside librpcc_hip.so: its directory, its public header and the directories
    of headers it shares with other side libraries (csrc_tile/: error state and tile preparation; csrc_lzmatch/: the match
    finder of the two entropy coders), so that neither DEPS nor source_digest() -- the compression library's identity --
    changes with it, and an edit of a shared header rebuilds every library that includes it."""
    deps = [os.path.join(_HERE, d, f) for d in (subdir,) + tuple(shared) for f in sorted(os.listdir(os.path.join(_HERE, d)))]
    return (os.path.join(_HERE, subdir, src), deps + [os.path.join(os.path.dirname(_HERE), "include", header)],
            os.path.join(_HERE, "lib", lib))


EVAL_SRC, EVAL_DEPS, EVAL_LIB = _side_library("csrc_eval", "eval_kernels.hip", "rpcc_eval.h", "librpcc_eval.so")   # reconstruction metrics
SEG_SRC, SEG_DEPS, SEG_LIB = _side_library("csrc_seg", "dbscan_kernels.hip", "rpcc_seg.h", "librpcc_seg.so")     # DBSCAN segmentation
_LZ = ("csrc_tile", "csrc_lzmatch")
LZ4_SRC, LZ4_DEPS, LZ4_LIB = _side_library("csrc_lz4", "lz4_kernels.hip", "rpcc_lz4.h", "librpcc_lz4.so", _LZ)   # LZ4 entropy back-end
DEFLATE_SRC, DEFLATE_DEPS, DEFLATE_LIB = _side_library("csrc_deflate", "deflate_kernels.hip", "rpcc_deflate.h", "librpcc_deflate.so", _LZ)   # gzip back-end
INFLATE_SRC, INFLATE_DEPS, INFLATE_LIB = _side_library("csrc_inflate", "inflate_kernels.hip", "rpcc_inflate.h", "librpcc_inflate.so")   # gzip decoder
BUNZIP2_SRC, BUNZIP2_DEPS, BUNZIP2_LIB = _side_library("csrc_bunzip2", "bunzip2_kernels.hip", "rpcc_bunzip2.h", "librpcc_bunzip2.so")   # bzip2 decoder
BZIP2_SRC, BZIP2_DEPS, BZIP2_LIB = _side_library("csrc_bzip2", "bzip2_kernels.hip", "rpcc_bzip2.h", "librpcc_bzip2.so")   # bzip2 encoder
FILTER_SRC, FILTER_DEPS, FILTER_LIB = _side_library("csrc_filter", "radius_filter.hip", "rpcc_filter.h", "librpcc_filter.so")   # radius outlier removal
RANS_SRC, RANS_DEPS, RANS_LIB = _side_library("csrc_rans", "rans_kernels.hip", "rpcc_rans.h", "librpcc_rans.so")   # chunk-parallel rANS back-end
RECORDS_SRC, RECORDS_DEPS, RECORDS_LIB = _side_library("csrc_records", "records_kernels.hip", "rpcc_records.h", "librpcc_records.so")   # NCLT record unpack
ROWS_SRC, ROWS_DEPS, ROWS_LIB = _side_library("csrc_rows", "rows_kernels.hip", "rpcc_rows.h", "librpcc_rows.so")   # decoded batch -> .bin rows
FIELDS_SRC, FIELDS_DEPS, FIELDS_LIB = _side_library("csrc_fields", "fields_kernels.hip", "rpcc_fields.h", "librpcc_fields.so")   # .pcd / .ply record unpack
CLOUD_SRC, CLOUD_DEPS, CLOUD_LIB = _side_library("csrc_cloud", "cloud_kernels.hip", "rpcc_cloud.h", "librpcc_cloud.so")   # image + hidden points -> .bin rows

# -ffp-contract=off: the reference's C++ (projection, models, prediction, quantisation) is un-fused x86 SSE arithmetic and a
# contracted FMA changes results.  (The reference's CUDA FPS kernel is a different matter: nvcc contracts its distance into
# FMAs by default; the build's FPS follows its own un-fused specification, see DESIGN.md section 2 "parity unpinned".)
HIPCC_FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fno-fast-math", "-fPIC",
               "-shared", "-Wno-unused-value"]


def source_digest():
    """sha256 over the sources librpcc_hip.so is built from (csrc/*, include/rpcc_hip.h; names and bytes, sorted): what a committed set of
    profiler counters (profiles/pmc_current*.json) is tied to -- bench.py prints no counter-derived fraction for another build."""
    import hashlib
    h = hashlib.sha256()
    for d in DEPS:
        h.update(os.path.basename(d).encode() + b"\0")
        h.update(open(d, "rb").read())
        h.update(b"\0")
    return h.hexdigest()


def build_host(force=False, verbose=False):
    """librpcc_host.so: the plain-C container packer (bzip2 through the libbz2 the interpreter's bz2 module links) and the LZF decoder of
    .pcd binary_compressed bodies."""
    os.makedirs(os.path.dirname(HOST_LIB), exist_ok=True)
    if not force and os.path.exists(HOST_LIB) and all(os.path.getmtime(HOST_LIB) >= os.path.getmtime(d) for d in [HOST_SRC] + HOST_LZF_DEPS):
        return HOST_LIB
    cmd = [os.environ.get("CC", "gcc"), "-O2", "-shared", "-fPIC", "-Wall", HOST_SRC, HOST_LZF_SRC, "-o", HOST_LIB, "-l:libbz2.so.1.0"]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return HOST_LIB


def _hipcc(src, lib, deps, force, verbose):
    os.makedirs(os.path.dirname(lib), exist_ok=True)
    if not force and os.path.exists(lib) and all(os.path.getmtime(lib) >= os.path.getmtime(d) for d in deps):
        return lib
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    extra = os.environ.get("RPCC_EXTRA_FLAGS", "").split()   # developer builds only: -DRPCC_DEVTRACE (csrc/rpcc_trace.h)
    cmd = [hipcc] + HIPCC_FLAGS + extra + [src, "-o", lib]
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return lib


def build_eval(force=False, verbose=False):
    """librpcc_eval.so: the reconstruction-metrics kernels (csrc_eval/), same flags and the same mtime rule as librpcc_hip.so."""
    return _hipcc(EVAL_SRC, EVAL_LIB, EVAL_DEPS, force, verbose)


def build_seg(force=False, verbose=False):
    """librpcc_seg.so: the DBSCAN segmentation kernels (csrc_seg/), same flags and the same mtime rule as librpcc_hip.so."""
    return _hipcc(SEG_SRC, SEG_LIB, SEG_DEPS, force, verbose)


def build_lz4(force=False, verbose=False):
    """librpcc_lz4.so: the LZ4 encode / decode / container kernels (csrc_lz4/), same flags and the same mtime rule as librpcc_hip.so."""
    return _hipcc(LZ4_SRC, LZ4_LIB, LZ4_DEPS, force, verbose)


def build_deflate(force=False, verbose=False):
    """librpcc_deflate.so: the gzip / deflate encoder kernels (csrc_deflate/), same flags and the same mtime rule as librpcc_hip.so."""
    return _hipcc(DEFLATE_SRC, DEFLATE_LIB, DEFLATE_DEPS, force, verbose)


def build_inflate(force=False, verbose=False):
    """librpcc_inflate.so: the gzip / deflate decoder kernel (csrc_inflate/), same flags and the same mtime rule as librpcc_hip.so."""
    return _hipcc(INFLATE_SRC, INFLATE_LIB, INFLATE_DEPS, force, verbose)


def build_bunzip2(force=False, verbose=False):
    """librpcc_bunzip2.so: the bzip2 decoder kernel (csrc_bunzip2/), same flags and the same mtime rule as librpcc_hip.so."""
    return _hipcc(BUNZIP2_SRC, BUNZIP2_LIB, BUNZIP2_DEPS, force, verbose)


def build_bzip2(force=False, verbose=False):
    """librpcc_bzip2.so: the bzip2 encoder kernels (csrc_bzip2/), same flags and the same mtime rule as librpcc_hip.so."""
    return _hipcc(BZIP2_SRC, BZIP2_LIB, BZIP2_DEPS, force, verbose)


def build_filter(force=False, verbose=False):
    """librpcc_filter.so: the radius outlier removal kernels (csrc_filter/), same flags and the same mtime rule as librpcc_hip.so."""
    return _hipcc(FILTER_SRC, FILTER_LIB, FILTER_DEPS, force, verbose)


def build_rans(force=False, verbose=False):
    """librpcc_rans.so: the chunk-parallel rANS encode / decode kernels (csrc_rans/), same flags and the same mtime rule as librpcc_hip.so."""
    return _hipcc(RANS_SRC, RANS_LIB, RANS_DEPS, force, verbose)


def build_records(force=False, verbose=False):
    """librpcc_records.so: the NCLT record unpack kernel (csrc_records/), same flags and the same mtime rule as librpcc_hip.so."""
    return _hipcc(RECORDS_SRC, RECORDS_LIB, RECORDS_DEPS, force, verbose)


def build_rows(force=False, verbose=False):
    """librpcc_rows.so: the .bin row packer (csrc_rows/), same flags and the same mtime rule as librpcc_hip.so."""
    return _hipcc(ROWS_SRC, ROWS_LIB, ROWS_DEPS, force, verbose)


def build_fields(force=False, verbose=False):
    """librpcc_fields.so: the .pcd / .ply record unpack kernel (csrc_fields/), same flags and the same mtime rule as librpcc_hip.so."""
    return _hipcc(FIELDS_SRC, FIELDS_LIB, FIELDS_DEPS, force, verbose)


def build_cloud(force=False, verbose=False):
    """librpcc_cloud.so: the .bin row packer for frames with extra points (csrc_cloud/), same flags and the same mtime rule as librpcc_hip.so."""
    return _hipcc(CLOUD_SRC, CLOUD_LIB, CLOUD_DEPS, force, verbose)


def build(force=False, verbose=False):
    try:
        build_host(force, verbose)
    except (subprocess.CalledProcessError, OSError) as e:   # no libbz2.so.1.0 / no gcc: compress_utils.pack_frames then
        print("librpcc_host.so not built (%s): containers are packed by the interpreter's bz2 module" % e)  # takes the Python path
    build_eval(force, verbose)
    build_seg(force, verbose)
    build_lz4(force, verbose)
    build_deflate(force, verbose)
    build_inflate(force, verbose)
    build_bunzip2(force, verbose)
    build_bzip2(force, verbose)
    build_filter(force, verbose)
    build_rans(force, verbose)
    build_records(force, verbose)
    build_rows(force, verbose)
    build_fields(force, verbose)
    build_cloud(force, verbose)
    return _hipcc(SRC, LIB, DEPS, force, verbose)


if __name__ == "__main__":
    print(build(force=True, verbose=True))
