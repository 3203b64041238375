"""build.INCLUDES against the sources: for every device source the table lists exactly
the project's device files the source includes, directly or through one of them
(CPU only).  Device files are the .hip sources, the *_dev.h device headers and the
ensemble's launch header; a source whose stamp misses one of them is not rebuilt
when that file changes, and scripts/build_variant.py rebuilds by the same table.
"""
import os
import re

from stochquant_amd import build

INCLUDE = re.compile(r'^\s*#\s*include\s+"([^"]+)"', re.M)


def is_device_file(name):
    return name.endswith(".hip") or name.endswith("_dev.h") or name == "sq_phi4_ens_launch.h"


def quoted_includes(name):
    with open(os.path.join(build.CSRC, name)) as fh:
        return INCLUDE.findall(fh.read())


def device_closure(name):
    """The device files `name` includes, transitively (through any project file, device file or not)."""
    found, seen, todo = set(), {name}, [name]
    while todo:
        for inc in quoted_includes(todo.pop()):
            if "/" in inc or inc in seen or not os.path.exists(os.path.join(build.CSRC, inc)):
                continue
            seen.add(inc)
            todo.append(inc)
            if is_device_file(inc):
                found.add(inc)
    return found


def test_includes_is_a_dict_of_lists_of_existing_files():
    assert isinstance(build.INCLUDES, dict)
    for src, deps in build.INCLUDES.items():
        assert src in build.DEVICE_SOURCES, src
        assert isinstance(deps, list) and len(set(deps)) == len(deps), src
        for d in deps:
            assert os.path.exists(os.path.join(build.CSRC, d)), (src, d)


def test_includes_is_what_the_sources_include():
    for src in build.DEVICE_SOURCES:
        assert set(build.INCLUDES.get(src, [])) == device_closure(src), src


def test_device_headers_are_stamped_through_includes_alone():
    # a device header in HEADERS would rebuild every source, host sources too, when it changes
    assert not [h for h in build.HEADERS if is_device_file(h)]
    used = {d for deps in build.INCLUDES.values() for d in deps}
    on_disk = {f for f in os.listdir(build.CSRC) if is_device_file(f) and not f.endswith(".hip")}
    assert on_disk <= used, on_disk - used


def test_only_sq_phi4_hip_is_included_in_part():
    """No guard macro carves a .hip file up for an includer, except sq_phi4.hip's SQ_PHI4_KERNELS_ONLY."""
    for f in sorted(os.listdir(build.CSRC)):
        with open(os.path.join(build.CSRC, f)) as fh:
            text = fh.read()
        for m in re.finditer(r"\w*KERNELS?_ONLY\w*", text):
            assert m.group(0) == "SQ_PHI4_KERNELS_ONLY", (f, m.group(0))
        if "SQ_PHI4_KERNELS_ONLY" in text:
            assert f == "sq_phi4.hip" or "sq_phi4.hip" in quoted_includes(f), f


def test_one_compile_command_carries_the_per_source_flags():
    for src in build.DEVICE_SOURCES + build.HOST_SOURCES:
        cmd = build.compile_command(src)
        assert cmd[0] == build.HIPCC and cmd[-1] == os.path.join(build.CSRC, src) and cmd[-2] == "-c"
        for flag in build.COMMON + build.EXTRA_FLAGS.get(src, []) + [f"--offload-arch={build.ARCH}"]:
            assert flag in cmd, (src, flag)
    assert build.compile_command("sq_phi4_ens_mala.hip", "/x/y.hip")[-1] == "/x/y.hip"
    assert "-disable-machine-licm" in build.compile_command("sq_phi4_ens_hmc.hip", "/x/y.hip")
    assert "-disable-machine-licm" not in build.compile_command("sq_phi4_ens.hip")
