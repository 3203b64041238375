"""sq::Buf (csrc/sq_buf.h) owns every buffer of the phi^4 ensemble's handle.  This
CPU check instantiates it over a counting, malloc-backed policy that can fail
the next allocation, and requires: reserve within the capacity keeps the
pointer, growth gives a new block of the new capacity, a failed growth leaves
the buffer empty and a later reserve succeeds, both moves leave the source
empty and free the overwritten target, and destruction frees -- allocations and
frees match, and the leak checker finds nothing left.  Built as a host program
with the address and undefined-behaviour sanitizers; the header needs no HIP."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))


def test_buf_owns_grows_moves_and_frees(tmp_path):
    exe = str(tmp_path / "buf_check")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-o", exe, os.path.join(HERE, "buf_check.cpp")], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "allocs 10 frees 10 bad 0" in r.stdout
