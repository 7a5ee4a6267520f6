"""Host: pass 1 of fast_nms_queue_ordered.  fast_queue_survivor (evh_detect_fast.h) is __host__ __device__; the stand-alone
program tools/fast_tail_host_check.hip includes the header, runs the function over random score planes with ties and compares
the survivor bitmap with the strict-maximum definition (halo, 31-pixel border rule, levels not larger than 62 included).  It is
built for the host only, with the address and undefined-behaviour sanitizers, and run as a process of its own."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pass1_survivors_equal_the_definition(tmp_path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / "fast_tail_host_check")
    subprocess.check_call([hipcc, "--offload-host-only", "-O1", "-g", "-std=c++17", "-Wno-unused-function",
                           "-I", os.path.join(ROOT, "evenvizion_amd", "csrc"), "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", os.path.join(ROOT, "tools", "fast_tail_host_check.hip"), "-o", exe])
    out = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    print(out.stdout)
    assert out.returncode == 0 and "pass 1 host check ok" in out.stdout, out.stdout
