"""csrc/label_bytes.h -- the packed-word label compare that count_scan_kernel counts with -- built for the host (tests/label_bytes_host_main.cpp)
and held to a byte loop: every pair of label bytes against every label, random words, whole 16-pixel lanes.  Built once more with
-fsanitize=address,undefined (runtimes inside the program).  No GPU needed."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", [["-O1"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                                                      "-static-libasan", "-static-libubsan"]], ids=["plain", "sanitized"])
def test_packed_label_compare_equals_the_byte_loop(tmp_path, flags):
    exe = str(tmp_path / "label_bytes_host")
    subprocess.check_call([os.environ.get("CXX", "g++")] + flags + ["-std=c++17", "-I", os.path.join(ROOT, "r-pcc_amd", "csrc"),
                           os.path.join(ROOT, "tests", "label_bytes_host_main.cpp"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, text=True, check=True).stdout
    m = re.search(r"checked (\d+) bad (\d+)", out)
    assert m and int(m.group(1)) > 2 ** 24 and int(m.group(2)) == 0, out
