"""phi4_noise_consts (csrc/sq_noise_consts.h) gives the fused kernels the
Philox words that depend only on (key, step); this CPU check completes the
evaluation from those words -- for step s, and for step s+1 from step s's
carried prefix, re-keyed across a change of step_hi -- and requires the plain
ten-round function's output for 1000 random (key, step) over a few quads each,
step_lo = 0 and 0xFFFFFFFF and step_hi != 0 included.  Built as a host
program with the address and undefined-behaviour sanitizers.  The GPU side is
pinned by tests/test_gpu_noise_carry.py."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_noise_consts_complete_philox(tmp_path):
    exe = str(tmp_path / "noise_consts_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "noise_consts_check.cpp")], check=True)
    r = subprocess.run([exe, "1000"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "checked 4000 bad 0" in r.stdout
