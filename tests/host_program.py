"""The stand-alone host programs of the CPU tier: ``tests/host_<stem>_main.cpp`` compiles a kernel's ``*_core.h`` for the host and is run
directly as a program of its own; nothing of it is ever loaded into Python."""
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def cxx():
    for cand in (os.environ.get("CXX"), "c++", "g++", "clang++"):
        if cand and shutil.which(cand):
            return [shutil.which(cand)]
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")  # what the library itself is built with; host-only C++ here
    assert os.path.exists(hipcc), "no host C++ compiler found (c++ / g++ / clang++ / hipcc)"
    return [hipcc, "-x", "c++"]


def build(tmp_path_factory, stem, *, sanitize, fp_contract_off=False, debug=None, timeout=600):
    """``host_<stem>`` in a directory of its own, from ``-O1 -std=c++17``.  ``sanitize``: under the address and undefined-behaviour
    sanitizers, every finding fatal; ``debug`` (``-g``) goes with it unless said otherwise.  ``fp_contract_off``: fuse no multiply with
    an add, for the kernels whose ``*_core.h`` says the same to its own compiler."""
    exe = tmp_path_factory.mktemp(f"host_{stem}") / f"host_{stem}"
    flags = ["-O1"] + (["-g"] if (sanitize if debug is None else debug) else []) + ["-std=c++17"]
    flags += ["-ffp-contract=off"] if fp_contract_off else []
    flags += ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"] if sanitize else []
    includes = ["-I" + os.path.join(ROOT, "climate2weather_amd", "csrc"), "-I" + os.path.join(ROOT, "tests")]  # the cores; host_main.h
    subprocess.run(cxx() + flags + includes + [os.path.join(ROOT, "tests", f"host_{stem}_main.cpp"), "-o", str(exe)], check=True, timeout=timeout)
    return exe
