"""The one way the host tests build a stand-alone C++ program: a stand-in main of tests/kernel_standin (the kernels' code against
hip_standin.h, one thread per lane) or a host probe of a plan header.  With FS2_STANDIN_ASAN=1 it is built with
-fsanitize=address,undefined, with FS2_STANDIN_TSAN=1 (for the mains that ask: tsan=True) with -fsanitize=thread -- stand-alone host
programs, so a sanitizer never sees Python or a GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fastspeech2_amd", "csrc")
STANDIN = os.path.join(ROOT, "tests", "kernel_standin")


def sanitizer_flags(tsan=False):
    if tsan:
        return ["-fsanitize=thread", "-g"] if os.environ.get("FS2_STANDIN_TSAN") == "1" else []
    return ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-g"] if os.environ.get("FS2_STANDIN_ASAN") == "1" else []


def build(tmp_path_factory, source, flags=("-std=c++20", "-O1", "-pthread"), extra=(), tsan=False):
    """Compile `source` (a path below the repository root) into a fresh directory -> the executable's path."""
    cxx = os.environ.get("CXX", "g++")
    if shutil.which(cxx) is None:
        pytest.fail("no C++ compiler (%s) to build %s" % (cxx, source))
    name = os.path.splitext(os.path.basename(source))[0]
    exe = str(tmp_path_factory.mktemp(name) / name)
    subprocess.run([cxx] + list(flags) + list(extra) + sanitizer_flags(tsan) + ["-I", os.path.join(ROOT, "include"), "-I", CSRC, "-I", STANDIN,
                                                                                 os.path.join(ROOT, source), "-o", exe], check=True)
    return exe
