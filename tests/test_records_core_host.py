"""csrc_records/records_rule.h, the text the gfx950 unpack kernel is compiled from, built for the host (tests/records_host_main.cpp)
and held to tests/records_ref.py on all 65 536 values of each field: the same bits, the sign of zero at the origin included.  Built
as the libraries are (-ffp-contract=off); with contraction allowed on a target that has a fused multiply-add, where the header's own
statement must keep the two roundings; and as the libraries are with -fsanitize=address,undefined, the runtimes inside the program.
No GPU needed."""
import os
import subprocess

import numpy as np
import pytest

import records_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_has_fma():
    try:
        with open("/proc/cpuinfo") as f:
            return any(line.startswith("flags") and " fma" in line for line in f)
    except OSError:
        return False


# (on a CPU without the instruction the second build only allows contraction; it cannot be run with -mfma there)
FMA_FLAGS = ["-O2", "-ffp-contract=fast"] + (["-mfma"] if _cpu_has_fma() else [])


SANITIZED = ["-O1", "-ffp-contract=off", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan"]


@pytest.mark.parametrize("flags", (["-O1", "-ffp-contract=off"], FMA_FLAGS, SANITIZED), ids=("unfused", "fma-allowed", "sanitized"))
def test_host_build_of_the_rule_equals_the_reference(tmp_path, flags):
    exe = str(tmp_path / "records_host")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17"] + flags +
                          ["-I", os.path.join(ROOT, "r-pcc_amd", "csrc_records"), os.path.join(ROOT, "tests", "records_host_main.cpp"), "-o", exe])
    recs = np.concatenate([R.field_sweep(f) for f in range(3)])
    recs.tofile(tmp_path / "in.bin")
    run = subprocess.run([exe, str(tmp_path / "in.bin"), str(tmp_path / "out.bin")], stderr=subprocess.PIPE)
    assert run.returncode == 0 and not run.stderr, run.stderr.decode(errors="replace")[-4000:]
    got = np.fromfile(tmp_path / "out.bin", dtype=np.float32).reshape(-1, 4)
    want = R.unpack_ref(recs)
    assert got.shape == want.shape
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert got.view(np.uint32)[20000, 0] == 0      # +0.0 at the origin
