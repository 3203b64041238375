"""Build libstochquant.so with a patched copy of one device file, for A/B runs
(SQ_LIB=<path> selects it at load time).

    python scripts/build_variant.py <patched file> <name> [replaced file, default sq_phi4.hip]
      -> stochquant_amd/lib/variants/libstochquant_<name>.so

The replaced file is a device source or a device header of build.INCLUDES.  Every
device source that is the file or whose INCLUDES entry names it is compiled again,
with its own flags (build.compile_command), in a copy of csrc/ that holds the
patched file under the replaced one's name; the other objects are the base build's.
"""
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from stochquant_amd import build  # noqa: E402


def dependents(which):
    """The device sources to rebuild when `which` changes, in DEVICE_SOURCES order."""
    return [s for s in build.DEVICE_SOURCES if s == which or which in build.INCLUDES.get(s, [])]


def main():
    src, name = sys.argv[1], sys.argv[2]
    which = sys.argv[3] if len(sys.argv) > 3 else "sq_phi4.hip"
    again = dependents(which)
    assert again, which
    build.build()
    tmp = os.path.join(build.OBJ, "variants", name)
    tree = os.path.join(tmp, "csrc")
    shutil.rmtree(tree, ignore_errors=True)
    shutil.copytree(build.CSRC, tree)  # quoted includes resolve beside the including file: the patched one
    shutil.copy(src, os.path.join(tree, which))
    objs = {}
    for s in again:
        objs[s] = os.path.join(tmp, s + ".o")
        # -I: the copy stands two levels deeper than csrc/, out of reach of its "../../include/..." includes
        subprocess.run(build.compile_command(s, os.path.join(tree, s)) + ["-I", build.CSRC, "-o", objs[s]], check=True)
    link = [objs.get(s, os.path.join(build.OBJ, s + ".o")) for s in build.DEVICE_SOURCES + build.HOST_SOURCES] \
        + [os.path.join(build.OBJ, "sq_build_id.cpp.o")]  # the base build's identity
    out = os.path.join(build.LIBDIR, "variants", f"libstochquant_{name}.so")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    subprocess.run([build.HIPCC, f"--offload-arch={build.ARCH}", "-shared", "-fPIC", "-o", out] + link
                   + [f"-L{build.ROCM}/lib", "-lrccl", f"-Wl,-rpath,{build.ROCM}/lib"], check=True)
    print(out)


if __name__ == "__main__":
    main()
