"""Host: the bit-plane segment test of k_fast_main's reference-order path.  bp_planes_item, bp_segment32, bp_range_mask and
fast_corner_px (evh_detect_fast.h) are __host__ __device__; the stand-alone program tools/fast_bitplane_host_check.hip includes
the header, emulates v_perm, v_alignbit and v_bitop3, walks levels tile by tile the way the kernel does and compares the corner
mask and the polarity mask, pixel for pixel, with the definition (nine contiguous ring pixels all below centre - 20 or all above
centre + 20): uniform noise, centres 0 .. 20 and 235 .. 255, ring values exactly centre +- 20 and +- 21, arcs of exactly 8 and 9
from every ring index, corners in the group columns 0, 1, 2, 29, 30, 31, levels no wider than one group and levels whose
testable range ends inside one.  It is built for the host only, with the address and undefined-behaviour sanitizers, and run as a
process of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plane_segment_test_equals_the_definition(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "fast_bitplane_host_check")
    subprocess.check_call([hipcc, "--offload-host-only", "-O1", "-g", "-std=c++17", "-Wno-unused-function",
                           "-I", os.path.join(ROOT, "evenvizion_amd", "csrc"), "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "fast_bitplane_host_check.hip"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "bit-plane host check ok" in out.stdout, out.stdout
